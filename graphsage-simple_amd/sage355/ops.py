"""Tensor-level wrappers of the C ABI operators (include/sage355.h).

Each function checks device / dtype / contiguity on the host -- a kernel that
walks a bad pointer can take the whole GPU node down -- then passes raw device
pointers to libsage355.  All work is enqueued on torch's current stream.
"""
import collections

import torch

from . import native
from .native import ACT_NONE, ACT_RELU, ACT_SIGMOID, TAG_INNER, TAG_INNER_SELF, TAG_OUTER  # noqa: F401


def _need_gpu():
    if not torch.cuda.is_available():
        raise native.SageError("sage355 needs an MI355X (torch.cuda.is_available() is False); there is no CPU path")


def _chk(t, dtype, name, dims=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise native.SageError(f"{name}: expected a device tensor")
    if t.dtype != dtype:
        raise native.SageError(f"{name}: dtype {t.dtype}, expected {dtype}")
    if not t.is_contiguous():
        raise native.SageError(f"{name}: must be contiguous")
    if dims is not None and t.dim() != dims:
        raise native.SageError(f"{name}: {t.dim()}-d, expected {dims}-d")
    return t


def _row_major(t, name, dtypes=(torch.float32,)):
    """2-d, unit inner stride, fp32 unless the caller allows more; returns (tensor, leading dimension in elements)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype not in dtypes or t.dim() != 2:
        raise native.SageError(f"{name}: expected a 2-d fp32 device tensor")
    if t.stride(1) != 1 and t.shape[1] > 1:
        raise native.SageError(f"{name}: inner stride must be 1")
    return t, (t.stride(0) if t.shape[0] > 1 else max(t.shape[1], 1))


def _feature_table(t, name):
    """The frozen feature table of the full-neighbourhood mean: fp32 or bf16 (a storage format: sage_csr_mean_bf16).  Everything
    else stays fp32 only."""
    return _row_major(t, name, (torch.float32, torch.bfloat16))


def _opt_i32(t, name, dims=None, min_len=None):
    """An optional int32 side array (n_dev, any_nonempty, slot_rows, self_row, self_index, self_nodes): None passes through."""
    if t is not None:
        _chk(t, torch.int32, name, dims)
        if min_len is not None and t.numel() < min_len:
            raise native.SageError(f"{name}: {t.numel()} entries, expected at least {min_len}")
    return t


def _sets(who, nbr, cnt, n_dev=None, slot_rows=None, self_row=None, any_nonempty=None):
    """The sampled sets of n rows (nbr int32 [n, k], cnt int32 [n]) and the side arrays that go with them; returns (n, k)."""
    _chk(nbr, torch.int32, "nbr", 2)
    _chk(cnt, torch.int32, "cnt", 1)
    n, k = nbr.shape
    if cnt.shape[0] < n:
        raise native.SageError(f"{who}: cnt has {cnt.shape[0]} entries for {n} sets")
    _opt_i32(n_dev, "n_dev", min_len=1)
    _opt_i32(slot_rows, "slot_rows", 1)
    _opt_i32(self_row, "self_row", 1, n)
    _opt_i32(any_nonempty, "any_nonempty", min_len=1)
    return n, k


def _graph(who, rowptr, col, rowptr_name="rowptr", col_name="col"):
    """The CSR pair every graph operator takes: rowptr int64 [rows + 1], col int32; returns the number of rows."""
    _chk(rowptr, torch.int64, rowptr_name, 1)
    _chk(col, torch.int32, col_name, 1)
    if rowptr.shape[0] < 1:
        raise native.SageError(f"{who}: {rowptr_name} is empty")
    return rowptr.shape[0] - 1


def _out_rows(who, out, rows, dim, device):
    """`out` of an operator that stores [rows, dim] fp32: a fresh one, or the caller's (row-major, at least `rows` rows, `dim`
    columns); returns (out, leading dimension)."""
    if out is None:
        out = torch.empty((rows, dim), dtype=torch.float32, device=device)
    out, ld = _row_major(out, "out")
    if out.shape[0] < rows or out.shape[1] != dim:
        raise native.SageError(f"{who}: out is {tuple(out.shape)}, expected ({rows}, {dim})")
    return out, ld


def _is_workspace(t, device):
    return isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and t.device == device and t.is_contiguous()


def _workspace(who, need, workspace, device, shape):
    """The workspace of a call that needs `need` bytes (0: `shape`, the caller's words for its sizes, is out of range): the caller's
    uint8 tensor on `device` when it is large enough, else a fresh one -- trainers hand every call one shared buffer that may be short."""
    if need == 0:
        raise native.SageError(f"{who}: {shape} out of range")
    if workspace is not None and not _is_workspace(workspace, device):
        raise native.SageError(f"{who}: workspace must be a uint8 tensor on {device}")
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, dtype=torch.uint8, device=device)
    return workspace


def _nonempty(t):
    """An empty tensor may have no storage address: the kernels read none of it, so zeros with one row (one element) stand in."""
    if t is None or t.numel() > 0:
        return t
    return torch.zeros([max(s, 1) for s in t.shape], dtype=t.dtype, device=t.device)


def refuse_bf16(t, who):
    """A path that has no bf16 form says so by name, instead of failing on whatever reads the table first."""
    if isinstance(t, torch.Tensor) and t.dtype == torch.bfloat16:
        raise native.SageError(f"{who}: a torch.bfloat16 table is not supported here (bf16 is a storage format of the frozen table of the "
                               "full-neighbourhood mean: ops.csr_mean, inference, ExactBatchTrainer, FullGraphTrainer(gcn=True)); pass table.float()")


def check_id_range(ids64, num_nodes, what="node ids"):
    """Host-side range check of ids that arrived from the host (numpy int64 array).  The reference fails safely for a
    bad id (IndexError from the nn.Embedding lookup, encoders.py:50 / aggregators.py:65); a device kernel would read
    rowptr[] out of bounds, so the check happens here, BEFORE the int32 cast can wrap a large id into range."""
    if num_nodes is not None:
        _in_range(what, "id", ids64, int(num_nodes))


def _in_range(who, what, values, k):
    """Every value (a numpy array or a tensor) inside [0, k), or SageError.  Host reads: for ids that come from the host and for
    what is built once per graph, never for a per-step wrapper."""
    if (values.numel() if isinstance(values, torch.Tensor) else values.size) == 0:
        return
    lo, hi = int(values.min()), int(values.max())
    if lo < 0 or hi >= k:
        raise native.SageError(f"{who}: {what} {lo if lo < 0 else hi} outside [0, {k})")


def _group_rowptr(keys, k):
    """int64 [k + 1]: the row pointer of k groups over entries sorted by their int64 group `keys` (bincount, cumsum)."""
    rowptr = torch.zeros(k + 1, dtype=torch.int64, device=keys.device)
    if k > 0 and keys.numel() > 0:
        rowptr[1:] = torch.cumsum(torch.bincount(keys, minlength=k), 0)
    return rowptr


def as_ids(nodes, device, num_nodes=None):
    """list / numpy / tensor of node ids -> int32 device tensor (encoders.py:40-47 accepts all three).
    num_nodes: ids that come from the HOST are range-checked against it (SageError); device-resident ids are not
    (that would be a host sync per call) -- the sampler kernels treat an out-of-range id as an isolated node instead."""
    import numpy as np
    if isinstance(nodes, torch.Tensor):
        if not nodes.is_cuda:
            check_id_range(nodes.detach().to(torch.int64).numpy(), num_nodes)
        return nodes.to(device=device, dtype=torch.int32).contiguous()
    ids64 = np.asarray(nodes, dtype=np.int64)
    check_id_range(ids64, num_nodes)
    return torch.from_numpy(np.ascontiguousarray(ids64.astype(np.int32))).to(device)


def next_pow2(x):
    p = 4
    while p < x:
        p <<= 1
    return p


def _frontier_struct(frontier):
    """The sage_frontier_t (`.c`) of a frontier -- a Frontier, or any object with its `keys` tensor and `c` -- for one call: its pointers
    were taken once, so the device rule (native.on_current_device) is checked again at every call that passes it."""
    native.on_current_device(frontier.keys)
    return frontier.c


class Frontier:
    """Device hash set of distinct ids + id -> row map (aggregators.py:52-53)."""

    def __init__(self, max_ids, device, first_row=0):
        _need_gpu()
        self.capacity = next_pow2(2 * max(int(max_ids), 1))
        self.max_nodes = int(max_ids) + int(first_row)
        self.keys = torch.empty(self.capacity, dtype=torch.int32, device=device)
        self.rows = torch.empty(self.capacity, dtype=torch.int32, device=device)
        self.nodes = torch.empty(self.max_nodes, dtype=torch.int32, device=device)
        self.count = torch.zeros(1, dtype=torch.int32, device=device)
        P = native.ptr                                     # the struct's pointers pass the one check too
        self.c = native.Frontier(P(self.keys).value, P(self.rows).value, self.capacity, P(self.nodes).value, P(self.count).value, self.max_nodes)
        self.reset(first_row)

    def reset(self, first_row=0):
        native.check(native.lib().sage_frontier_reset(_frontier_struct(self), int(first_row), native.stream_handle()), "frontier_reset")

    def size(self):
        return int(self.count.item())   # host sync: tests / generic path only

    def node_list(self):
        return self.nodes[: self.size()]


def _sample(entry, rowptr, col, nodes, k, seed, tag, n_dev, frontier, insert_self, any_nonempty, out_nbr, out_cnt):
    """Body of the two sampler wrappers: `entry` names the C entry point (same argument list)."""
    _need_gpu()
    num_nodes = _graph(entry, rowptr, col)
    _chk(nodes, torch.int32, "nodes", 1)
    _opt_i32(n_dev, "n_dev", min_len=1)
    _opt_i32(any_nonempty, "any_nonempty", min_len=1)
    n = nodes.shape[0]
    dev = nodes.device
    nbr = torch.empty((n, k), dtype=torch.int32, device=dev) if out_nbr is None else _chk(out_nbr, torch.int32, "out_nbr")
    cnt = torch.empty(n, dtype=torch.int32, device=dev) if out_cnt is None else _chk(out_cnt, torch.int32, "out_cnt")
    if nbr.numel() < n * k or cnt.numel() < n:
        raise native.SageError(f"{entry}: output buffers too small")
    nbr_slot = torch.empty((n, k), dtype=torch.int32, device=dev) if frontier is not None else None
    self_slot = torch.empty(n, dtype=torch.int32, device=dev) if (frontier is not None and insert_self) else None
    rc = getattr(native.lib(), "sage_" + entry)(
        native.ptr(rowptr), native.ptr(col), num_nodes, native.ptr(nodes), n, native.ptr(n_dev), int(k),
        int(seed) & 0xFFFFFFFFFFFFFFFF, int(tag), native.ptr(nbr), native.ptr(cnt), native.ptr(any_nonempty),
        _frontier_struct(frontier) if frontier is not None else None, 1 if insert_self else 0, native.ptr(nbr_slot),
        native.ptr(self_slot), native.stream_handle())
    native.check(rc, entry)
    return nbr, cnt, nbr_slot, self_slot


def sample_neighbors(rowptr, col, nodes, k, seed, tag=TAG_OUTER, n_dev=None, frontier=None, insert_self=False,
                     any_nonempty=None, out_nbr=None, out_cnt=None):
    """encoders.py:47 + aggregators.py:42-48 (+52-53 with a frontier), k <= native.MAX_FANOUT.
    -> (nbr int32 [n,k], cnt int32 [n], nbr_slot or None, self_slot or None)."""
    return _sample("sample_neighbors", rowptr, col, nodes, k, seed, tag, n_dev, frontier, insert_self, any_nonempty, out_nbr, out_cnt)


def sample_neighbors_wide(rowptr, col, nodes, k, seed, tag=TAG_OUTER, n_dev=None, frontier=None, insert_self=False,
                          any_nonempty=None, out_nbr=None, out_cnt=None):
    """The same hop for any k <= native.MAX_FANOUT_WIDE (sage_sample_neighbors_wide: one wave per node).  Same draw: for
    k <= native.MAX_FANOUT the outputs equal sample_neighbors' bit for bit."""
    return _sample("sample_neighbors_wide", rowptr, col, nodes, k, seed, tag, n_dev, frontier, insert_self, any_nonempty, out_nbr, out_cnt)


def sample_neighbors_any(rowptr, col, nodes, k, seed, tag=TAG_OUTER, n_dev=None, frontier=None, insert_self=False,
                         any_nonempty=None, out_nbr=None, out_cnt=None):
    """sample_neighbors for k <= native.MAX_FANOUT (a lane per slot: at small k several nodes share a wave), sample_neighbors_wide above."""
    entry = "sample_neighbors" if int(k) <= native.MAX_FANOUT else "sample_neighbors_wide"
    return _sample(entry, rowptr, col, nodes, k, seed, tag, n_dev, frontier, insert_self, any_nonempty, out_nbr, out_cnt)


def frontier_insert(nbr, cnt, frontier, self_nodes=None, n_dev=None):
    _need_gpu()
    n, k = _sets("frontier_insert", nbr, cnt, n_dev)
    _opt_i32(self_nodes, "self_nodes", 1, n)
    nbr_slot = torch.empty_like(nbr)
    self_slot = torch.empty(n, dtype=torch.int32, device=nbr.device) if self_nodes is not None else None
    rc = native.lib().sage_frontier_insert(native.ptr(nbr), native.ptr(cnt), k, native.ptr(self_nodes), n,
                                           native.ptr(n_dev), _frontier_struct(frontier), native.ptr(nbr_slot), native.ptr(self_slot),
                                           native.stream_handle())
    native.check(rc, "frontier_insert")
    return nbr_slot, self_slot


def gather_mean(table, nbr, cnt, slot_rows=None, self_row=None, any_nonempty=None, n_dev=None, out=None):
    """aggregators.py:54-74 -> [n, dim] mean of the gathered rows."""
    _need_gpu()
    table, ld = _row_major(table, "table")
    n, k = _sets("gather_mean", nbr, cnt, n_dev, slot_rows, self_row, any_nonempty)
    dim = table.shape[1]
    out, ldo = _out_rows("gather_mean", out, n, dim, table.device)
    rc = native.lib().sage_gather_mean(native.ptr(table), table.shape[0], ld, dim, native.ptr(nbr), native.ptr(cnt), k, n,
                                       native.ptr(n_dev), native.ptr(slot_rows), native.ptr(self_row),
                                       native.ptr(any_nonempty), native.ptr(out), ldo, native.stream_handle())
    native.check(rc, "gather_mean")
    return out


def gather_mean_backward(grad_out, nbr, cnt, table_rows, slot_rows=None, self_row=None, n_dev=None, out=None):
    """The adjoint of gather_mean with respect to its table, [table_rows, dim], by fp32 atomic scatter (sage_gather_mean_backward:
    the order of additions is not fixed; the engine's reproducible form is sage_gather_mean_backward_ws).  grad_out [n, dim] = d loss /
    d gather_mean's result; nbr, cnt, slot_rows, self_row as the forward took them.  ACCUMULATES into out (zeros when absent)."""
    _need_gpu()
    grad_out, ldg = _row_major(grad_out, "grad_out")
    n, k = _sets("gather_mean_backward", nbr, cnt, n_dev, slot_rows, self_row)
    rows, dim = int(table_rows), grad_out.shape[1]
    if grad_out.shape[0] < n:
        raise native.SageError(f"gather_mean_backward: grad_out has {grad_out.shape[0]} rows for {n} sets")
    if out is None:
        out = torch.zeros((rows, dim), dtype=torch.float32, device=grad_out.device)
    out, ld = _out_rows("gather_mean_backward", out, rows, dim, grad_out.device)
    rc = native.lib().sage_gather_mean_backward(native.ptr(grad_out), ldg, dim, native.ptr(nbr), native.ptr(cnt), k, n, native.ptr(n_dev),
                                                native.ptr(slot_rows), native.ptr(self_row), native.ptr(out), rows, ld,
                                                native.stream_handle())
    native.check(rc, "gather_mean_backward")
    return out


def _linear_inputs(who, agg, weight, self_tab, self_index, n_dev):
    """What linear_act and its backward read: agg [n, dim], weight [out_dim, dim | 2 dim] over [self | agg], self_tab [*, dim] and the
    int32 arrays; returns the leading dimensions (agg, weight, self_tab or 0)."""
    _, ld_agg = _row_major(agg, "agg")
    _, ldw = _row_major(weight, "weight")
    n, dim = agg.shape
    ld_self = 0
    if self_tab is not None:
        _, ld_self = _row_major(self_tab, "self_tab")
        if self_tab.shape[1] != dim:
            raise native.SageError(f"{who}: self_tab width != agg width")
    if weight.shape[1] != dim * (2 if self_tab is not None else 1):
        raise native.SageError(f"{who}: weight is {tuple(weight.shape)}, inputs are {dim} wide")
    _opt_i32(self_index, "self_index", 1, n)
    _opt_i32(n_dev, "n_dev", min_len=1)
    return ld_agg, ldw, ld_self


def linear_act(agg, weight, act=ACT_RELU, self_tab=None, self_index=None, n_dev=None, out=None):
    """encoders.py:49-62 -> [n, out_dim] (the module hands out the transpose view)."""
    _need_gpu()
    ld_agg, ldw, ld_self = _linear_inputs("linear_act", agg, weight, self_tab, self_index, n_dev)
    (n, dim), out_dim = agg.shape, weight.shape[0]
    out, ldo = _out_rows("linear_act", out, n, out_dim, agg.device)
    rc = native.lib().sage_linear_act(native.ptr(self_tab), ld_self, native.ptr(self_index), native.ptr(agg), ld_agg, dim,
                                      native.ptr(weight), ldw, out_dim, int(act), n, native.ptr(n_dev), native.ptr(out),
                                      ldo, native.stream_handle())
    native.check(rc, "linear_act")
    return out


def linear_act_backward_workspace_bytes(n, dim, has_self, out_dim):
    """Bytes of the workspace sage_linear_act_backward_ws needs for its weight gradient (host arithmetic)."""
    return int(native.lib().sage_linear_act_backward_workspace_bytes(int(n), int(dim), int(bool(has_self)), int(out_dim)))


def linear_act_backward(agg, weight, act, out, grad_out, self_tab=None, self_index=None, n_dev=None, need_w=True, need_x=True,
                        workspace=None):
    """The backward of linear_act over its n rows (the first n_dev[0] of them when given) -> (grad_w, grad_x), either None when not
    asked for.  out is what the forward returned, grad_out = d loss / d out; grad_w has weight's shape, grad_x [n, kw] is
    d loss / d [self | agg].  The reproducible entry point (sage_linear_act_backward_ws): the partial tiles of grad_w go through a
    workspace and are added in a fixed order, no float atomics.  workspace: a uint8 device tensor to use when it is large enough."""
    _need_gpu()
    ld_agg, ldw, ld_self = _linear_inputs("linear_act_backward", agg, weight, self_tab, self_index, n_dev)
    n, dim = agg.shape
    out_dim, kw = weight.shape
    lds = []
    for t, name in ((out, "out"), (grad_out, "grad_out")):
        lds.append(_row_major(t, name)[1])
        if t.shape[0] < n or t.shape[1] < out_dim:
            raise native.SageError(f"linear_act_backward: {name} is {tuple(t.shape)}, expected at least ({n}, {out_dim})")
    grad_w = torch.zeros_like(weight) if need_w else None
    grad_x = torch.empty((n, kw), dtype=torch.float32, device=agg.device) if need_x else None
    ws = None
    if need_w:
        need = max(256, linear_act_backward_workspace_bytes(n, dim, self_tab is not None, out_dim))
        ws = _workspace("linear_act_backward", need, workspace, agg.device, "")
    P = native.ptr
    rc = native.lib().sage_linear_act_backward_ws(
        P(self_tab), ld_self, P(self_index), P(agg), ld_agg, dim, P(weight), ldw, out_dim, int(act), P(out), lds[0], P(grad_out), lds[1],
        n, P(n_dev), P(grad_w), grad_w.stride(0) if need_w else 0, P(grad_x), kw if need_x else 0, None,
        P(ws), ws.numel() if need_w else 0, native.stream_handle())
    native.check(rc, "linear_act_backward")
    return grad_w, grad_x


class Scratch:
    """Named uint8 buffers of one device that only ever grow: get(name, nbytes) -> a buffer of at least nbytes (256 at the least),
    the same one as long as it is large enough."""

    def __init__(self, device):
        self.device, self._buffers = device, {}

    def get(self, name, nbytes):
        t = self._buffers.get(name)
        if t is None or t.numel() < nbytes:
            t = self._buffers[name] = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=self.device)
        return t


def layer_forward_supported(dim, out_dim, concat):
    return bool(native.lib().sage_layer_forward_supported(int(dim), int(out_dim), 1 if concat else 0))


def layer_forward(table, nbr, cnt, weight, act=ACT_RELU, concat=False, self_index=None, slot_rows=None, self_row=None,
                  any_nonempty=None, n_dev=None, out=None):
    """One Encoder.forward (encoders.py:47-62) in one launch."""
    _need_gpu()
    table, ld = _row_major(table, "table")
    weight, ldw = _row_major(weight, "weight")
    n, k = _sets("layer_forward", nbr, cnt, n_dev, slot_rows, self_row, any_nonempty)
    _opt_i32(self_index, "self_index", 1, n)
    dim = table.shape[1]
    out_dim = weight.shape[0]
    if weight.shape[1] != dim * (2 if concat else 1):
        raise native.SageError(f"layer_forward: weight is {tuple(weight.shape)}, table is {dim} wide")
    out, ldo = _out_rows("layer_forward", out, n, out_dim, table.device)
    rc = native.lib().sage_layer_forward(native.ptr(table), table.shape[0], ld, dim, native.ptr(nbr), native.ptr(cnt), k, n,
                                         native.ptr(n_dev), native.ptr(slot_rows), native.ptr(self_row),
                                         native.ptr(any_nonempty), 1 if concat else 0, native.ptr(self_index),
                                         native.ptr(weight), ldw, out_dim, int(act), native.ptr(out), ldo,
                                         native.stream_handle())
    native.check(rc, "layer_forward")
    return out


def slice_major(table, slice_floats=32):
    """[N, D] -> the slice-major copy float[D / W][N][W] (sage_model_t.table_sliced)."""
    n, d = table.shape
    if d % slice_floats:
        raise native.SageError(f"slice_major: {d} columns are not whole slices of {slice_floats}")
    return table.view(n, d // slice_floats, slice_floats).permute(1, 0, 2).contiguous()


def prepare_weights(weight, concat=False):
    """W [out_dim, dim | 2 dim] -> its bf16 planes in the contraction kernels' register order (sage_prepare_weights)."""
    _need_gpu()
    weight, ldw = _row_major(weight, "weight")
    out_dim, dim = weight.shape[0], weight.shape[1] // (2 if concat else 1)
    need = native.lib().sage_prepared_weight_bytes(dim, out_dim, int(bool(concat)))
    if need == 0:
        raise native.SageError(f"prepare_weights: no prepared form for dim={dim} out_dim={out_dim}")
    prep = torch.empty(need, dtype=torch.uint8, device=weight.device)
    native.check(native.lib().sage_prepare_weights(native.ptr(weight), ldw, dim, out_dim, int(bool(concat)), native.ptr(prep), need,
                                                   native.stream_handle()), "prepare_weights")
    return prep


def layer1_fused_supported(dim, out_dim, k):
    return bool(native.lib().sage_layer1_fused_supported(int(dim), int(out_dim), int(k)))


def layer1_fused(table_sliced, nbr, cnt, weight, act=ACT_RELU, self_row=None, any_nonempty=None, n_dev=None, out=None, prepared=None):
    """The gcn encoder's layer 1 in one phase-sliced launch on a slice-major table float[D / 32][N][32] (sage_layer1_fused)."""
    _need_gpu()
    if not (isinstance(table_sliced, torch.Tensor) and table_sliced.is_cuda and table_sliced.dim() == 3 and table_sliced.shape[2] == 32
            and table_sliced.is_contiguous() and table_sliced.dtype == torch.float32):
        raise native.SageError("layer1_fused: table_sliced must be a contiguous fp32 [D / 32, N, 32] device tensor")
    weight, ldw = _row_major(weight, "weight")
    n, k = _sets("layer1_fused", nbr, cnt, n_dev, None, self_row, any_nonempty)
    dim, rows = table_sliced.shape[0] * 32, table_sliced.shape[1]
    out_dim = weight.shape[0]
    if weight.shape[1] != dim:
        raise native.SageError(f"layer1_fused: weight is {tuple(weight.shape)}, table is {dim} wide")
    if prepared is None:
        prepared = prepare_weights(weight)
    elif not _is_workspace(prepared, weight.device):
        raise native.SageError("layer1_fused: prepared must be what prepare_weights returns for this weight")
    out, ldo = _out_rows("layer1_fused", out, n, out_dim, table_sliced.device)
    rc = native.lib().sage_layer1_fused(native.ptr(table_sliced), rows, dim, native.ptr(nbr), native.ptr(cnt), k, n, native.ptr(n_dev),
                                        native.ptr(self_row), native.ptr(any_nonempty), native.ptr(weight), ldw, native.ptr(prepared),
                                        out_dim, int(act), native.ptr(out), ldo, native.stream_handle())
    native.check(rc, "layer1_fused")
    return out


def csr_mean_workspace_bytes(n, max_edges, dim):
    """Bytes of the workspace sage_csr_mean needs (host arithmetic; 0 = shape out of range)."""
    return int(native.lib().sage_csr_mean_workspace_bytes(int(n), int(max_edges), int(dim)))


def csr_mean(rowptr, col, table, nodes=None, self_loop=False, any_nonempty=None, out=None, max_edges=None, workspace=None, index=None):
    """aggregators.py:47-48 (num_sample=None) + 52-74 from the CSR: [n, dim] mean over every neighbour of each node
    (row r is node nodes[r], or node r without `nodes`).  max_edges: upper bound on the edges of the selected rows, default
    len(col) (exact for distinct rows; a smaller bound only costs speed).  workspace: a uint8 device tensor to reuse.
    index: int32 [num_nodes] on the device -- `table` is then a [K, dim] embedding and node v's row is table[index[v]]
    (aggregators.py:68-71; sage_csr_mean_indexed): the bits of csr_mean(table[index]) without that [num_nodes, dim] array.  An
    index value outside [0, K) is clamped, not refused: check the index where it is built.
    table may be torch.bfloat16 (sage_csr_mean_bf16; not with index=): the caller rounded it once, the kernel widens each element
    exactly and sums in fp32, so the result is csr_mean(table.float()) bit for bit at half the table bytes; out stays fp32."""
    _need_gpu()
    num_nodes = _graph("csr_mean", rowptr, col)
    if index is not None:
        refuse_bf16(table, "csr_mean(index=): the embedding is trained and stays fp32")
    table, ld = _feature_table(table, "table")
    if index is not None:
        _chk(index, torch.int32, "index", 1)
        if index.shape[0] != num_nodes or table.shape[0] < 1:
            raise native.SageError(f"csr_mean: index has {index.shape[0]} entries for {num_nodes} nodes, the embedding {table.shape[0]} rows")
    elif table.shape[0] < max(num_nodes, 1):
        raise native.SageError(f"csr_mean: table has {table.shape[0]} rows for {num_nodes} nodes")
    if nodes is not None:
        _chk(nodes, torch.int32, "nodes", 1)
    n = num_nodes if nodes is None else nodes.shape[0]
    dim = table.shape[1]
    out, ldo = _out_rows("csr_mean", out, n, dim, table.device)
    _opt_i32(any_nonempty, "any_nonempty", min_len=1)
    if n == 0:
        return out
    col, index = _nonempty(col), _nonempty(index)
    max_edges = col.numel() if max_edges is None else int(max_edges)
    workspace = _workspace("csr_mean", csr_mean_workspace_bytes(n, max_edges, dim), workspace, table.device,
                           f"n = {n}, max_edges = {max_edges}, dim = {dim}")
    lib, P = native.lib(), native.ptr
    graph = (P(rowptr), P(col), num_nodes, P(nodes), n, max_edges)
    rest = (P(table), table.shape[0], ld, dim, 1 if self_loop else 0, P(any_nonempty), P(out), ldo, P(workspace), workspace.numel(),
            native.stream_handle())
    if index is not None:
        native.check(lib.sage_csr_mean_indexed(*graph, P(index), *rest), "csr_mean_indexed")
    elif table.dtype == torch.bfloat16:
        native.check(lib.sage_csr_mean_bf16(*graph, *rest), "csr_mean_bf16")
    else:
        native.check(lib.sage_csr_mean(*graph, *rest), "csr_mean")
    return out


def csr_frontier_workspace_bytes(n, max_edges):
    """Bytes of the workspace sage_csr_frontier needs (host arithmetic; 0 = shape out of range)."""
    return int(native.lib().sage_csr_frontier_workspace_bytes(int(n), int(max_edges)))


class CsrFrontier:
    """The state of sage_csr_frontier for one graph: `pos` int32 [num_nodes], the id -> row map (filled with -1 ONCE, here; clear()
    afterwards takes back the rows that were handed out and nothing else), `nodes` int32 [max_nodes], `count` int32 [1] and a workspace
    that grows with the calls.  max_nodes: rows of `nodes` (default num_nodes, which no set outgrows); reserve() grows it.
    pos is what csr_mean(index=...) and linear_act(self_index=...) take to read compact rows by node id."""

    def __init__(self, num_nodes, device, max_nodes=None):
        _need_gpu()
        self.num_nodes = int(num_nodes)
        self.max_nodes = self.num_nodes if max_nodes is None else int(max_nodes)
        if self.num_nodes < 0 or self.num_nodes >= 1 << 31 or self.max_nodes < 0:
            raise native.SageError(f"CsrFrontier: num_nodes = {num_nodes}, max_nodes = {max_nodes}")
        self.pos = torch.full((max(self.num_nodes, 1),), -1, dtype=torch.int32, device=device)
        self.nodes = torch.full((max(self.max_nodes, 1),), -1, dtype=torch.int32, device=device)
        self.count = torch.zeros(1, dtype=torch.int32, device=device)
        self.workspace = None

    def reserve(self, max_nodes):
        """Room for max_nodes rows in `nodes`; the rows it holds are kept."""
        max_nodes = int(max_nodes)
        if max_nodes > self.nodes.numel():
            grown = torch.full((max_nodes,), -1, dtype=torch.int32, device=self.nodes.device)
            grown[: self.nodes.numel()] = self.nodes
            self.nodes = grown
        self.max_nodes = max(self.max_nodes, max_nodes)

    def clear(self, first_row=0):
        """pos := -1 where this frontier's rows point (sage_csr_frontier_clear, no O(num_nodes) fill), count := first_row."""
        native.check(native.lib().sage_csr_frontier_clear(native.ptr(self.pos), native.ptr(self.nodes), native.ptr(self.count),
                                                          min(self.max_nodes, self.nodes.numel()), native.stream_handle()), "csr_frontier_clear")
        self.count.fill_(int(first_row))

    def refill(self):
        """pos := -1 everywhere, count := 0: after an overflow, when `nodes` no longer names every row of pos."""
        self.pos.fill_(-1)
        self.count.zero_()

    def size(self):
        return int(self.count.item())   # host read

    def node_list(self):
        n = self.size()
        if n > self.max_nodes:
            raise native.SageError(f"CsrFrontier: {n} rows for max_nodes = {self.max_nodes}")
        return self.nodes[:n]


def csr_frontier(rowptr, col, seeds, frontier, max_edges=None):
    """aggregators.py:47-53 with num_sample=None, from the CSR: every distinct id among `seeds` (int32, device; may repeat) and all
    their neighbours joins `frontier` (a CsrFrontier of this graph, cleared) -- frontier.nodes[:count] in arbitrary order,
    frontier.pos[id] = its row.  max_edges: upper bound on the edges of the seeds' rows, default len(col) (a smaller bound only costs
    speed).  Nothing is read back: frontier.size() is the host read, and a size above frontier.max_nodes means the set did not fit."""
    _need_gpu()
    num_nodes = _graph("csr_frontier", rowptr, col)
    _chk(seeds, torch.int32, "seeds", 1)
    if not isinstance(frontier, CsrFrontier):
        raise native.SageError("csr_frontier: frontier must be a CsrFrontier")
    if num_nodes != frontier.num_nodes:
        raise native.SageError(f"csr_frontier: the frontier maps {frontier.num_nodes} nodes, the CSR has {num_nodes}")
    n = seeds.shape[0]
    if n == 0:
        return frontier
    dev = frontier.pos.device
    col = _nonempty(col)
    max_edges = col.numel() if max_edges is None else int(max_edges)
    frontier.workspace = _workspace("csr_frontier", csr_frontier_workspace_bytes(n, max_edges), frontier.workspace, dev,
                                    f"n = {n}, max_edges = {max_edges}")
    rc = native.lib().sage_csr_frontier(native.ptr(rowptr), native.ptr(col), num_nodes, native.ptr(seeds), n, max_edges,
                                        native.ptr(frontier.pos), native.ptr(frontier.nodes), min(frontier.max_nodes, frontier.nodes.numel()),
                                        native.ptr(frontier.count), native.ptr(frontier.workspace), frontier.workspace.numel(),
                                        native.stream_handle())
    native.check(rc, "csr_frontier")
    return frontier


def csr_transpose(rowptr, col):
    """(rowptr_t int64 [N + 1], col_t int32 [E]) of a CSR over N = len(rowptr) - 1 nodes: for every entry (v -> u) row u of the
    transpose holds one entry v, in ascending v (duplicates kept) -- what csr_mean_backward sums over.  Torch ops (a stable sort by
    destination, bincount, cumsum) on the tensors' own device, CPU or GPU; built once per graph.  An id outside [0, N) raises:
    the differentiable path needs ids inside the graph (one check here, at build time)."""
    if not isinstance(rowptr, torch.Tensor) or not isinstance(col, torch.Tensor) or rowptr.dim() != 1 or col.dim() != 1:
        raise native.SageError("csr_transpose: rowptr and col must be 1-d tensors")
    n = rowptr.shape[0] - 1
    if n < 0:
        raise native.SageError("csr_transpose: rowptr is empty")
    rp = rowptr.to(torch.int64)
    e = int(rp[-1]) if n > 0 else 0
    if e < 0 or e > col.numel() or int(rp[0]) != 0 or (n > 0 and bool((rp[1:] < rp[:-1]).any())):
        raise native.SageError("csr_transpose: rowptr is not a row pointer array of col")
    dst = col[:e].to(torch.int64)
    _in_range("csr_transpose", "id", dst, n)
    src = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=col.device), rp[1:] - rp[:-1])
    order = torch.sort(dst, stable=True).indices                 # sources are ascending already: stable keeps them so inside a row
    return _group_rowptr(dst, n), src[order].to(torch.int32)


def csr_mean_backward_workspace_bytes(num_nodes, n, max_edges, dim):
    """Bytes of the workspace sage_csr_mean_backward needs (host arithmetic; 0 = shape out of range)."""
    return int(native.lib().sage_csr_mean_backward_workspace_bytes(int(num_nodes), int(n), int(max_edges), int(dim)))


def csr_mean_backward(rowptr, col, rowptr_t, col_t, grad_out, nodes=None, self_loop=False, out=None, max_edges=None, workspace=None):
    """The adjoint of csr_mean(rowptr, col, table) (every node) with respect to `table`: [n, dim], row r the gradient of table
    row nodes[r] (row r without `nodes`).  (rowptr_t, col_t) = csr_transpose(rowptr, col).  grad_out [num_nodes, dim], by node id.
    The result is stored, not accumulated.  max_edges: upper bound on the entries of the selected transposed rows, default
    len(col_t) (exact for distinct rows; a smaller bound only costs speed).  workspace: a uint8 device tensor to reuse."""
    _need_gpu()
    num_nodes = _graph("csr_mean_backward", rowptr, col)
    _graph("csr_mean_backward", rowptr_t, col_t, "rowptr_t", "col_t")
    grad_out, ldg = _row_major(grad_out, "grad_out")
    if rowptr_t.shape[0] != rowptr.shape[0] or col_t.numel() != col.numel():
        raise native.SageError("csr_mean_backward: the transpose does not have the graph's shape")
    if grad_out.shape[0] < num_nodes:
        raise native.SageError(f"csr_mean_backward: grad_out has {grad_out.shape[0]} rows for {num_nodes} nodes")
    if nodes is not None:
        _chk(nodes, torch.int32, "nodes", 1)
    n = num_nodes if nodes is None else nodes.shape[0]
    dim = grad_out.shape[1]
    out, ldgt = _out_rows("csr_mean_backward", out, n, dim, grad_out.device)
    if n == 0:
        return out
    col, col_t = _nonempty(col), _nonempty(col_t)
    max_edges = col_t.numel() if max_edges is None else int(max_edges)
    workspace = _workspace("csr_mean_backward", csr_mean_backward_workspace_bytes(num_nodes, n, max_edges, dim), workspace, grad_out.device,
                           f"n = {n}, max_edges = {max_edges}, dim = {dim}")
    rc = native.lib().sage_csr_mean_backward(native.ptr(rowptr), native.ptr(col), native.ptr(rowptr_t), native.ptr(col_t), num_nodes,
                                             native.ptr(nodes), n, max_edges, native.ptr(grad_out), ldg, dim, 1 if self_loop else 0,
                                             native.ptr(out), ldgt, native.ptr(workspace), workspace.numel(), native.stream_handle())
    native.check(rc, "csr_mean_backward")
    return out


GroupedTranspose = collections.namedtuple("GroupedTranspose", "rowptr col self_loop")


def csr_transpose_grouped(rowptr, col, index, num_groups, self_loop=False):
    """GroupedTranspose(rowptr_gt int64 [K + 1], col_gt int32 [E + S], self_loop) -- what csr_mean_backward_grouped sums over for
    an embedding [K = num_groups, dim] read as embed[index[v]] through csr_mean(..., index=index).  Row k lists, for every node u
    with index[u] == k in ascending u, the entries of row u of the transpose (csr_transpose's order) and then u itself if u joins
    its own mean (self_loop and u not an entry of its own row): S such self entries in all.  Torch ops on the tensors' own device,
    CPU or GPU (the transpose, then ONE stable sort by (index[owner], owner) of the transposed entries with the self entries
    appended); built once per graph, like csr_transpose and group_rows.  Raises for an index value outside [0, K), a node id
    outside the graph and len(index) != N.  The flag travels with the list: the backward cannot be run with another one."""
    if not isinstance(index, torch.Tensor) or index.dim() != 1 or index.dtype not in (torch.int32, torch.int64):
        raise native.SageError("csr_transpose_grouped: index must be a 1-d int32 / int64 tensor")
    rowptr_t, col_t = csr_transpose(rowptr, col)                       # checks rowptr and the ids in col
    n, k = rowptr.shape[0] - 1, int(num_groups)
    dev = col_t.device
    if index.shape[0] != n or index.device != dev:
        raise native.SageError(f"csr_transpose_grouped: index has {index.shape[0]} entries on {index.device} for {n} nodes on {dev}")
    if k < 0 or k >= (1 << 31):
        raise native.SageError(f"csr_transpose_grouped: num_groups = {k}")
    idx = index.to(torch.int64)
    _in_range("csr_transpose_grouped", "index", idx, k)
    nodes = torch.arange(n, dtype=torch.int64, device=dev)
    owner = torch.repeat_interleave(nodes, rowptr_t[1:] - rowptr_t[:-1])           # col_t's rows: ascending already
    entry = col_t.to(torch.int64)
    if self_loop and n > 0:
        own = torch.zeros(n, dtype=torch.bool, device=dev)
        own[owner[entry == owner]] = True                                           # u is an entry of its own row
        selfs = nodes[~own]
        owner, entry = torch.cat([owner, selfs]), torch.cat([entry, selfs])         # appended: stable keeps them last in their node
    order = torch.sort(idx[owner] * max(n, 1) + owner, stable=True).indices
    return GroupedTranspose(_group_rowptr(idx[owner], k), entry[order].to(torch.int32), bool(self_loop))


def csr_mean_backward_grouped_workspace_bytes(num_nodes, num_groups, max_edges, dim):
    """Bytes of the workspace sage_csr_mean_backward_grouped needs (host arithmetic; 0 = shape out of range)."""
    return int(native.lib().sage_csr_mean_backward_grouped_workspace_bytes(int(num_nodes), int(num_groups), int(max_edges), int(dim)))


def csr_mean_backward_grouped(rowptr, col, grouped, grad_out, out=None, max_edges=None, workspace=None):
    """The adjoint of csr_mean(rowptr, col, embed, index=index) (every node) with respect to `embed`: [K, dim], with no
    [num_nodes, dim] intermediate.  grouped = csr_transpose_grouped(rowptr, col, index, K, self_loop): it carries the flag.
    grad_out [num_nodes, dim], by node id.  The result is stored, not accumulated; an embedding row nobody reads is zeros.
    max_edges: upper bound on the list's entries, default len(grouped.col) (a smaller bound only costs speed).  workspace: a
    uint8 device tensor to reuse."""
    _need_gpu()
    if not isinstance(grouped, GroupedTranspose):
        raise native.SageError("csr_mean_backward_grouped: grouped must be what csr_transpose_grouped returns")
    num_nodes = _graph("csr_mean_backward_grouped", rowptr, col)
    rowptr_gt, col_gt = grouped.rowptr, grouped.col
    k = _graph("csr_mean_backward_grouped", rowptr_gt, col_gt, "grouped.rowptr", "grouped.col")
    grad_out, ldg = _row_major(grad_out, "grad_out")
    if not col.numel() <= col_gt.numel() <= col.numel() + num_nodes:
        raise native.SageError("csr_mean_backward_grouped: the grouped list does not have the graph's shape")
    if grad_out.shape[0] < num_nodes:
        raise native.SageError(f"csr_mean_backward_grouped: grad_out has {grad_out.shape[0]} rows for {num_nodes} nodes")
    dim = grad_out.shape[1]
    out, ldge = _out_rows("csr_mean_backward_grouped", out, k, dim, grad_out.device)
    if k == 0:
        return out
    if num_nodes == 0:                                    # no node reads any row
        out[:k].zero_()
        return out
    col, col_gt = _nonempty(col), _nonempty(col_gt)
    max_edges = grouped.col.numel() if max_edges is None else int(max_edges)
    workspace = _workspace("csr_mean_backward_grouped", csr_mean_backward_grouped_workspace_bytes(num_nodes, k, max_edges, dim), workspace,
                           grad_out.device, f"K = {k}, max_edges = {max_edges}, dim = {dim}")
    rc = native.lib().sage_csr_mean_backward_grouped(native.ptr(rowptr), native.ptr(col), native.ptr(rowptr_gt), native.ptr(col_gt),
                                                     num_nodes, k, max_edges, native.ptr(grad_out), ldg, dim, 1 if grouped.self_loop else 0,
                                                     native.ptr(out), ldge, native.ptr(workspace), workspace.numel(),
                                                     native.stream_handle())
    native.check(rc, "csr_mean_backward_grouped")
    return out


_SeedBatch = collections.namedtuple("_SeedBatch", "n dim rows max_edges device shape args keep")   # keep: the tensors `args` points into


def _seed_batch(who, rowptr, col, nodes, grad_out, index, num_rows, max_edges, total_terms):
    """The prologue of the two seed-batch adjoints (csr_mean_backward_rows / _touched): the checks of the graph, the seed rows, their
    gradient, the index with num_rows and total_terms; the ONE host read of the wrappers (max_edges=None: the entries of the seeds'
    rows); the stand-ins of empty arrays.  `args` are the leading arguments of both C entries (rowptr .. dim), `shape` the sizes in
    words for a refusal."""
    _need_gpu()
    num_nodes = _graph(who, rowptr, col)
    _chk(nodes, torch.int32, "nodes", 1)
    grad_out, ldg = _row_major(grad_out, "grad_out")
    n, dim = nodes.shape[0], grad_out.shape[1]
    if grad_out.shape[0] < n:
        raise native.SageError(f"{who}: grad_out has {grad_out.shape[0]} rows for {n} seed rows")
    if index is not None:
        _chk(index, torch.int32, "index", 1)
        if index.shape[0] != num_nodes:
            raise native.SageError(f"{who}: index has {index.shape[0]} entries for {num_nodes} nodes")
        if num_rows is None:
            raise native.SageError(f"{who}: num_rows is required with an index")
    rows = num_nodes if num_rows is None else int(num_rows)
    if rows < 0 or (rows == 0 and n > 0):
        raise native.SageError(f"{who}: num_rows = {rows} with {n} seed rows")
    if total_terms is not None:
        _chk(total_terms, torch.int64, "total_terms", 1)
    if max_edges is None:                                 # the host read: the entries of the seeds' rows (ids clamped into the graph)
        v = nodes.long().clamp_(0, max(num_nodes - 1, 0))
        max_edges = int((rowptr[v + 1] - rowptr[v]).clamp_(min=0).sum()) if n > 0 and num_nodes > 0 else 0
    max_edges = int(max_edges)
    P = native.ptr
    keep = col, nodes, index, grad_out = _nonempty(col), _nonempty(nodes), _nonempty(index), _nonempty(grad_out)
    args = (P(rowptr), P(col), num_nodes, P(nodes), n, max_edges, P(index), rows, P(grad_out), ldg, dim)
    return _SeedBatch(n, dim, rows, max_edges, grad_out.device, f"n = {n}, max_edges = {max_edges}, num_rows = {rows}, dim = {dim}", args, keep)


_TouchedOut = collections.namedtuple("_TouchedOut", "result args")


def _touched_out(who, n, dim, rows, cap, table, table_name, lr, want_grad, out, device, total_terms=None):
    """The output block of the two touched-rows entries (csr_mean_backward_touched / embed_grad_rows) over a table of `rows` rows:
    `table` (named table_name) and lr go together or the gradient is wanted; (rows, num_rows, grad_rows) of `cap` rows are the
    caller's `out` or fresh; without terms (n == 0) the library launches nothing, so the counts are zeroed here.  result = the
    triple to return, args = the C entries' arguments num_rows_out .. lr."""
    if not want_grad and table is None:
        raise native.SageError(f"{who}: nothing to do: want_grad=False and no {table_name} to update")
    if (table is None) != (lr is None):
        raise native.SageError(f"{who}: {table_name} and lr go together")
    ldt = 0
    if table is not None:
        table, ldt = _row_major(table, table_name)
        if table.shape[0] < rows or table.shape[1] != dim:
            raise native.SageError(f"{who}: {table_name} is {tuple(table.shape)}, expected ({rows}, {dim})")
    if want_grad and cap < 1 and n > 0:
        raise native.SageError(f"{who}: max_rows = {cap}")
    cap = max(cap, 1)
    rows_t, num_t, grad_t = out if out is not None else (None, None, None)
    if num_t is None:
        num_t = torch.empty(1, dtype=torch.int32, device=device)
    _chk(num_t, torch.int32, "num_rows", 1)
    ldr = 0
    if want_grad:
        if rows_t is None:
            rows_t = torch.empty(cap, dtype=torch.int32, device=device)
        if grad_t is None:
            grad_t = torch.empty((cap, dim), dtype=torch.float32, device=device)
        _chk(rows_t, torch.int32, "rows", 1)
        grad_t, ldr = _row_major(grad_t, "grad_rows")
        if rows_t.shape[0] < cap or grad_t.shape[0] < cap or grad_t.shape[1] != dim:
            raise native.SageError(f"{who}: out is rows {tuple(rows_t.shape)}, grad_rows {tuple(grad_t.shape)}, expected ({cap},) and "
                                   f"({cap}, {dim})")
    else:
        rows_t = grad_t = None
    if n == 0:
        num_t.zero_()
        if total_terms is not None:
            total_terms.zero_()
    P = native.ptr
    return _TouchedOut((rows_t, num_t, grad_t), (P(num_t), P(rows_t), P(grad_t), cap, ldr, P(table), ldt, 0.0 if lr is None else float(lr)))


def csr_mean_backward_rows_workspace_bytes(n, max_edges, num_rows, dim):
    """Bytes of the workspace sage_csr_mean_backward_rows needs (host arithmetic; 0 = shape out of range)."""
    return int(native.lib().sage_csr_mean_backward_rows_workspace_bytes(int(n), int(max_edges), int(num_rows), int(dim)))


def csr_mean_backward_rows(rowptr, col, nodes, grad_out, index=None, num_rows=None, self_loop=False, out=None, max_edges=None,
                           workspace=None, total_terms=None):
    """The adjoint of csr_mean(rowptr, col, table, nodes=nodes, index=index) with respect to `table`: [num_rows, dim], the
    gradient of every row of the table the seed batch read (sage_csr_mean_backward_rows: the batch's terms sorted by table row,
    512-term chunks, fixed order, no float atomics).  nodes: int32 [n] on the device, may repeat; grad_out [n, dim], by seed ROW.
    index: int32 [num_nodes] -- a frontier's id -> row map (CsrFrontier.pos) or an embedding index; num_rows = the table's rows,
    default num_nodes without an index, required with one.  Stored, not accumulated: a row nobody read is zeros.
    max_edges: upper bound on the entries of the seeds' rows; None costs one host read of their count.  A bound below the truth
    DROPS the terms past it: total_terms (int64 [1] on the device) receives the true term count (entries + self terms).
    workspace: a uint8 device tensor to reuse."""
    who = "csr_mean_backward_rows"
    b = _seed_batch(who, rowptr, col, nodes, grad_out, index, num_rows, max_edges, total_terms)
    out, ldgt = _out_rows(who, out, b.rows, b.dim, b.device)
    if b.rows == 0:
        return out
    workspace = _workspace(who, csr_mean_backward_rows_workspace_bytes(b.n, b.max_edges, b.rows, b.dim), workspace, b.device, b.shape)
    rc = native.lib().sage_csr_mean_backward_rows(*b.args, 1 if self_loop else 0, native.ptr(out), ldgt, native.ptr(total_terms),
                                                  native.ptr(workspace), workspace.numel(), native.stream_handle())
    native.check(rc, who)
    return out


def csr_mean_backward_touched_workspace_bytes(n, max_edges, num_rows, dim):
    """Bytes of the workspace sage_csr_mean_backward_touched needs (host arithmetic; 0 = shape out of range; one value for every
    num_rows >= max_edges + n)."""
    return int(native.lib().sage_csr_mean_backward_touched_workspace_bytes(int(n), int(max_edges), int(num_rows), int(dim)))


def csr_mean_backward_touched(rowptr, col, nodes, grad_out, index=None, num_rows=None, self_loop=False, max_edges=None, max_rows=None,
                              table=None, lr=None, want_grad=True, out=None, workspace=None, total_terms=None):
    """csr_mean_backward_rows for the touched table rows only, and / or their SGD update in place (sage_csr_mean_backward_touched:
    nothing sized by num_rows or the graph).  The first arguments, max_edges and total_terms are csr_mean_backward_rows'.
    -> (rows, num_rows, grad_rows): num_rows int32 [1] on the device, the number U of distinct table rows with a term; rows int32
    [max_rows], grad_rows [max_rows, dim]: the first min(U, max_rows) of them ascending and their sums, bit for bit the rows
    csr_mean_backward_rows stores (entries past that are left as they were); both None with want_grad=False.  max_rows: default
    min(max_edges + n, num_rows), which always holds every row.  table [num_rows, dim] with lr: table[e] = fma(-lr, sum, table[e])
    for ALL U rows, in place, other rows untouched (torch's version counter of `table` does not move: the caller's business).
    out: (rows, num_rows, grad_rows) to write into (rows / grad_rows may be None there with want_grad=False); workspace: a uint8
    device tensor to reuse."""
    who, P = "csr_mean_backward_touched", native.ptr
    b = _seed_batch(who, rowptr, col, nodes, grad_out, index, num_rows, max_edges, total_terms)
    t = _touched_out(who, b.n, b.dim, b.rows, min(b.max_edges + b.n, b.rows) if max_rows is None else int(max_rows), table, "table", lr,
                     want_grad, out, b.device, total_terms)
    if b.n == 0:
        return t.result
    workspace = _workspace(who, csr_mean_backward_touched_workspace_bytes(b.n, b.max_edges, b.rows, b.dim), workspace, b.device, b.shape)
    rc = native.lib().sage_csr_mean_backward_touched(*b.args, 1 if self_loop else 0, *t.args, P(total_terms), P(workspace), workspace.numel(),
                                                     native.stream_handle())
    native.check(rc, who)
    return t.result


def group_rows(index, num_groups):
    """(rowptr_g int64 [K + 1], col_g int32 [N]) of an index [N] with values in [0, K = num_groups): row k of this rectangular
    CSR holds the positions v with index[v] == k, ascending -- what csr_sum adds up for row k of a shared embedding
    (aggregators.py:68-71).  Torch ops (a stable sort, bincount, cumsum) on the index's own device, CPU or GPU; built once per
    graph, like csr_transpose.  A value outside [0, K) raises."""
    if not isinstance(index, torch.Tensor) or index.dim() != 1 or index.dtype not in (torch.int32, torch.int64):
        raise native.SageError("group_rows: index must be a 1-d int32 / int64 tensor")
    k = int(num_groups)
    if k < 0 or index.numel() >= (1 << 31):
        raise native.SageError(f"group_rows: num_groups = {k}, {index.numel()} positions")
    idx = index.to(torch.int64)
    _in_range("group_rows", "index", idx, k)
    col_g = torch.sort(idx, stable=True).indices.to(torch.int32)      # positions are ascending already: stable keeps them so inside a group
    return _group_rowptr(idx, k), col_g


def csr_sum_workspace_bytes(num_rows, max_edges, dim):
    """Bytes of the workspace sage_csr_sum needs (host arithmetic; 0 = shape out of range)."""
    return int(native.lib().sage_csr_sum_workspace_bytes(int(num_rows), int(max_edges), int(dim)))


def csr_sum(rowptr, col, table, out=None, max_edges=None, workspace=None):
    """[K, dim]: row r is the sum of table[col[e]] over row r's entries of the rectangular CSR (rowptr [K + 1], col) in stored
    order -- with (rowptr, col) = group_rows(index, K) the gradient of an embedding read as embed[index].  The result is stored,
    not accumulated; an empty row is zeros.  max_edges: upper bound on rowptr[-1], default len(col) (a smaller bound only costs
    speed).  workspace: a uint8 device tensor to reuse."""
    _need_gpu()
    num_rows = _graph("csr_sum", rowptr, col)
    table, ld = _row_major(table, "table")
    if table.shape[0] < 1:
        raise native.SageError("csr_sum: table has no rows")
    dim = table.shape[1]
    out, ldo = _out_rows("csr_sum", out, num_rows, dim, table.device)
    if num_rows == 0:
        return out
    col = _nonempty(col)
    max_edges = col.numel() if max_edges is None else int(max_edges)
    workspace = _workspace("csr_sum", csr_sum_workspace_bytes(num_rows, max_edges, dim), workspace, table.device,
                           f"num_rows = {num_rows}, max_edges = {max_edges}, dim = {dim}")
    rc = native.lib().sage_csr_sum(native.ptr(rowptr), native.ptr(col), num_rows, max_edges, native.ptr(table), table.shape[0], ld, dim,
                                   native.ptr(out), ldo, native.ptr(workspace), workspace.numel(), native.stream_handle())
    native.check(rc, "csr_sum")
    return out


def pagerank_workspace_bytes(num_nodes, num_edges):
    """Bytes of the workspace the sage_pagerank_* entries need (host arithmetic; 0 = shape out of range)."""
    return int(native.lib().sage_pagerank_workspace_bytes(int(num_nodes), int(num_edges)))


def _pagerank_graph(who, rowptr, col, alpha):
    """The pull CSR of a PageRank call and its alpha; returns (N, col with an address, number of edges the workspace is sized for)."""
    _need_gpu()
    n = _graph(who, rowptr, col)
    if n < 1:
        raise native.SageError(f"{who}: the graph has no nodes")
    if not 0.0 < float(alpha) < 1.0:
        raise native.SageError(f"{who}: alpha = {alpha!r}, expected inside (0, 1)")
    return n, _nonempty(col), col.numel()


def pagerank_step(rowptr, col, x, inv_out, alpha=0.85, workspace=None):
    """One PageRank power-iteration step from any x: (x_next float32 [N], err float32 [1] on the device) with
    x_next = alpha * (pull of x * inv_out over the CSR + mass / N) + (1 - alpha) / N, mass = the sum of x over the dangling nodes
    (inv_out == 0), err = sum |x_next - x|, N = len(x) (include/sage355.h: sage_pagerank_load, sage_pagerank_step).  Row i of
    (rowptr, col) lists the nodes that link to i; inv_out is 1 / out-degree, 0 for a dangling node."""
    n, col, e = _pagerank_graph("pagerank_step", rowptr, col, alpha)
    _chk(x, torch.float32, "x", 1)
    _chk(inv_out, torch.float32, "inv_out", 1)
    if x.shape[0] != n or inv_out.shape[0] != n:
        raise native.SageError(f"pagerank_step: x has {x.shape[0]} and inv_out {inv_out.shape[0]} entries for {n} nodes")
    dev = x.device
    workspace = _workspace("pagerank_step", pagerank_workspace_bytes(n, e), workspace, dev, f"num_nodes = {n}, num_edges = {e}")
    y, x_next, y_next = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(3))
    state = torch.empty(2, dtype=torch.float32, device=dev)
    L, st = native.lib(), native.stream_handle()
    native.check(L.sage_pagerank_load(native.ptr(rowptr), n, e, native.ptr(x), native.ptr(inv_out), native.ptr(y), native.ptr(state),
                                      native.ptr(workspace), workspace.numel(), st), "pagerank_load")
    native.check(L.sage_pagerank_step(native.ptr(rowptr), native.ptr(col), n, e, native.ptr(inv_out), float(alpha), native.ptr(x), native.ptr(y),
                                      native.ptr(x_next), native.ptr(y_next), native.ptr(state), native.ptr(workspace), workspace.numel(), st),
                 "pagerank_step")
    return x_next, state[:1]


def pagerank(rowptr, col, alpha=0.85, tol=1e-6, max_iter=100, symmetric=True, err_history=None):
    """(x float32 [N], iterations): nx.pagerank of the CSR graph with networkx's defaults (model.py:158-162 calls it so) -- uniform
    start, personalization and dangling weights, the power iteration stopped after the first step with err < N * tol; SageError
    naming "converge" after max_iter steps, where networkx raises PowerIterationFailedConvergence.  symmetric=True: the graph's
    own CSR is its pull CSR (every stored entry one link, a self loop too).  symmetric=False: rows are out-edge lists, as of an
    nx.DiGraph; the pull runs over csr_transpose(rowptr, col) with the out-degrees of the original rows.  Ids are checked once, on
    the host; per iteration the host reads the 4 bytes of err.  err_history: a list that receives every step's err."""
    n, col, _ = _pagerank_graph("pagerank", rowptr, col, alpha)
    if int(max_iter) < 1:
        raise native.SageError(f"pagerank: max_iter = {max_iter!r}")
    e = int(rowptr[-1])
    if e < 0 or e > col.numel() or int(rowptr[0]) != 0:
        raise native.SageError("pagerank: rowptr is not a row pointer array of col")
    dev = col.device
    out_degree = None
    if symmetric:
        _in_range("pagerank", "id", col[:e], n)
    else:
        out_degree = (rowptr[1:] - rowptr[:-1]).to(torch.int32).contiguous()
        rowptr, col = csr_transpose(rowptr, col)                      # checks the ids itself
        col = _nonempty(col)
    workspace = _workspace("pagerank", pagerank_workspace_bytes(n, e), None, dev, f"num_nodes = {n}, num_edges = {e}")
    xs, ys = torch.empty(2, n, dtype=torch.float32, device=dev), torch.empty(2, n, dtype=torch.float32, device=dev)
    inv_out = torch.empty(n, dtype=torch.float32, device=dev)
    state = torch.empty(2, dtype=torch.float32, device=dev)
    L, st = native.lib(), native.stream_handle()
    native.check(L.sage_pagerank_init(native.ptr(rowptr), n, e, native.ptr(out_degree), native.ptr(xs[0]), native.ptr(ys[0]), native.ptr(inv_out),
                                      native.ptr(state), native.ptr(workspace), workspace.numel(), st), "pagerank_init")
    for it in range(1, int(max_iter) + 1):
        cur, nxt = (it - 1) & 1, it & 1
        native.check(L.sage_pagerank_step(native.ptr(rowptr), native.ptr(col), n, e, native.ptr(inv_out), float(alpha), native.ptr(xs[cur]),
                                          native.ptr(ys[cur]), native.ptr(xs[nxt]), native.ptr(ys[nxt]), native.ptr(state), native.ptr(workspace),
                                          workspace.numel(), st), "pagerank_step")
        err = float(state[0])
        if err_history is not None:
            err_history.append(err)
        if err < n * tol:
            return xs[nxt].clone(), it
    raise native.SageError(f"pagerank: power iteration failed to converge within {int(max_iter)} iterations (err = {err:.3e}, "
                           f"N * tol = {n * tol:.3e})")


def csr_cheb_workspace_bytes(num_nodes, num_edges, dim):
    """Bytes of the workspace the sage_csr_cheb_* entries need (host arithmetic; 0 = shape out of range)."""
    return int(native.lib().sage_csr_cheb_workspace_bytes(int(num_nodes), int(num_edges), int(dim)))


class CsrChebPlan:
    """A square CSR graph planned for csr_cheb_step at one width: the chunk split of its long rows sits in `workspace`, made once by
    csr_cheb_plan and read by every step."""

    def __init__(self, rowptr, col, dim, num_nodes, num_edges, workspace):
        self.rowptr, self.col, self.dim, self.num_nodes, self.num_edges, self.workspace = rowptr, col, dim, num_nodes, num_edges, workspace


def csr_cheb_plan(rowptr, col, dim):
    """CsrChebPlan of the square CSR (rowptr int64 [N + 1], col int32) for blocks of `dim` columns (include/sage355.h:
    sage_csr_cheb_plan).  Once per graph and width; the steps on it re-plan nothing."""
    _need_gpu()
    n = _graph("csr_cheb_plan", rowptr, col)
    if n < 1:
        raise native.SageError("csr_cheb_plan: the graph has no nodes")
    dim = int(dim)
    col = _nonempty(col)
    e = col.numel()
    workspace = _workspace("csr_cheb_plan", csr_cheb_workspace_bytes(n, e, dim), None, col.device, f"num_nodes = {n}, num_edges = {e}, dim = {dim}")
    native.check(native.lib().sage_csr_cheb_plan(native.ptr(rowptr), n, e, dim, native.ptr(workspace), workspace.numel(), native.stream_handle()),
                 "csr_cheb_plan")
    return CsrChebPlan(rowptr, col, dim, n, e, workspace)


def csr_cheb_step(plan, y, x=None, a=1.0, b=0.0, g=0.0, out=None):
    """[N, dim]: out[i] = a * S_i + b * y[i] + g * x[i] with S_i the sum of y[col[e]] over row i's entries in stored order (the bits of
    csr_sum) -- one step of a Chebyshev three-term recurrence, or with the defaults the product A.y (include/sage355.h:
    sage_csr_cheb_step).  x=None drops the last term.  y, x and out are fp32 row-major with any leading dimension; out may be x
    (in place), never y."""
    _need_gpu()
    if not isinstance(plan, CsrChebPlan):
        raise native.SageError("csr_cheb_step: plan must come from csr_cheb_plan")
    n, dim = plan.num_nodes, plan.dim
    y, ldy = _row_major(y, "y")
    if tuple(y.shape) != (n, dim):
        raise native.SageError(f"csr_cheb_step: y is {tuple(y.shape)}, expected ({n}, {dim})")
    ldx = dim
    if x is not None:
        x, ldx = _row_major(x, "x")
        if tuple(x.shape) != (n, dim):
            raise native.SageError(f"csr_cheb_step: x is {tuple(x.shape)}, expected ({n}, {dim})")
    out, ldo = _out_rows("csr_cheb_step", out, n, dim, y.device)
    ws = plan.workspace
    rc = native.lib().sage_csr_cheb_step(native.ptr(plan.rowptr), native.ptr(plan.col), n, plan.num_edges, native.ptr(y), ldy, native.ptr(x), ldx,
                                         dim, float(a), float(b), float(g), native.ptr(out), ldo, native.ptr(ws), ws.numel(),
                                         native.stream_handle())
    native.check(rc, "csr_cheb_step")
    return out


EIGEN_MAX_K = 1000                                               # the reference's assert on feature_dim (model.py:165)


def _cholesky_qr(x, spare):
    """x [N, m] with orthonormal columns to about the square of its condition number times fp32 rounding: the Gram matrix by torch.mm
    on the device, its m x m Cholesky factor in fp64 on the host, x . R^-1 into `spare`.  A Gram matrix that is not positive definite
    in fp64 (columns dependent to rounding) goes through its eigen-decomposition instead, small eigenvalues raised to rounding level.
    Returns (the orthonormalised block, the buffer that is free now)."""
    import numpy as np
    gram = torch.mm(x.t(), x).double().cpu().numpy()
    gram = (gram + gram.T) / 2
    try:
        rinv = np.linalg.inv(np.linalg.cholesky(gram)).T
    except np.linalg.LinAlgError:
        w, q = np.linalg.eigh(gram)
        rinv = q / np.sqrt(np.maximum(w, w.max() * 2.0 ** -40))
    torch.mm(x, torch.from_numpy(np.ascontiguousarray(rinv)).to(device=x.device, dtype=torch.float32), out=spare)
    return spare, x


def _round_once(v):
    """v [N, k] fp32, orthonormal to the rounding of the fp32 products that made it (about sqrt(m) * 2^-24), orthonormalised once more
    in fp64 -- Gram matrix and product on the device, the k x k Cholesky factor on the host -- and rounded to fp32: what is returned
    is an orthonormal block rounded once, |V^T V - I| <= 2^-23 per element."""
    import numpy as np
    v64 = v.double()
    gram = torch.mm(v64.t(), v64).cpu().numpy()
    rinv = np.linalg.inv(np.linalg.cholesky((gram + gram.T) / 2)).T
    return torch.mm(v64, torch.from_numpy(np.ascontiguousarray(rinv)).to(v.device)).float()


def _fix_signs(v):
    """Each column's entry of largest magnitude made positive, the lowest index on a tie (in place)."""
    n, k = v.shape
    rows = torch.arange(n, dtype=torch.int32, device=v.device).unsqueeze(1)
    for c0 in range(0, k, 16):
        blk = v[:, c0:c0 + 16]
        mag = blk.abs()
        first = torch.where(mag == mag.amax(0, keepdim=True), rows, n).amin(0).long()
        lead = blk.gather(0, first.unsqueeze(0))
        blk.mul_(torch.where(lead < 0, -1.0, 1.0).to(v.dtype))
    return v


def eigen_top(rowptr, col, k, tol=1e-4, max_iter=200, degree=10, guard=None, seed=0, check_symmetric=True, history=None):
    """(values float64 [k] on the host, descending; vectors float32 [N, k] on the device; iterations): the k largest eigenvalues of the
    symmetric CSR graph's adjacency matrix (every stored entry a 1) and their eigenvectors -- what model.py:163-180 takes from a dense
    LA.eig -- by Chebyshev-filtered subspace iteration on a block of m = k + guard columns.  Every A.X is one csr_cheb_step on a
    graph planned once; the dense algebra (Gram matrices, rotations) is torch.mm on the device, the m x m Cholesky and eigh fp64
    on the host.  Every returned pair has ||A v - theta v||_2 <= tol * theta_1 as evaluated here in fp32; columns are orthonormal
    to one fp32 rounding (a last fp64 pass, _round_once) and their entry of largest magnitude is positive (lowest index on a tie); the same arguments give the same bits.
    SageError: k outside [1, min(N, 1000)], no entries, a CSR that is not symmetric (check_symmetric: one comparison with
    csr_transpose), no convergence within max_iter outer iterations ("converge").  history: a list that receives each iteration's
    largest residual norm of the first k pairs."""
    import math

    import numpy as np
    k = int(k)
    if k < 1 or k > EIGEN_MAX_K:
        raise native.SageError(f"eigen_top: k = {k}, expected inside [1, {EIGEN_MAX_K}]")
    if int(max_iter) < 1 or int(degree) < 1 or not float(tol) > 0.0:
        raise native.SageError(f"eigen_top: max_iter = {max_iter!r}, degree = {degree!r}, tol = {tol!r}")
    if guard is not None and int(guard) < 0:
        raise native.SageError(f"eigen_top: guard = {guard!r}")
    _need_gpu()
    n = _graph("eigen_top", rowptr, col)
    if k > n:
        raise native.SageError(f"eigen_top: k = {k} for a graph of {n} nodes")
    e = int(rowptr[-1])
    if e < 0 or e > col.numel() or int(rowptr[0]) != 0:
        raise native.SageError("eigen_top: rowptr is not a row pointer array of col")
    if e == 0:
        raise native.SageError("eigen_top: the graph has no entries (every eigenvalue is 0)")
    dev = col.device
    lens = rowptr[1:] - rowptr[:-1]
    if bool((lens < 0).any()):
        raise native.SageError("eigen_top: rowptr is not a row pointer array of col")
    _in_range("eigen_top", "id", col[:e], n)
    src = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=dev), lens)
    dst = col[:e].to(torch.int64)
    if check_symmetric:
        rowptr_t, col_t = csr_transpose(rowptr, col[:e])          # row u: its sources, ascending
        own = torch.sort(src * n + dst).values % n                 # row u: its stored ids, ascending
        if not torch.equal(rowptr_t, rowptr) or not torch.equal(own.to(torch.int32), col_t):
            raise native.SageError("eigen_top: the CSR is not symmetric (row u must hold v as often as row v holds u)")
    # rho(A)^2 <= the largest row sum of A^2 = max_i sum over row i's entries of len(col[e]): a proven lower bound of the spectrum
    lo = -math.sqrt(float(torch.zeros(n, dtype=torch.int64, device=dev).index_add_(0, src, lens[dst]).max()))
    del src, dst
    m = k + (max(8, k // 5) if guard is None else int(guard))
    m = min(n, (m + 3) // 4 * 4)
    plan = csr_cheb_plan(rowptr, col, m)
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(seed))
    x = torch.randn(n, m, generator=gen, device=dev, dtype=torch.float32)
    b1, b2, b3 = (torch.empty_like(x) for _ in range(3))
    theta = None
    for it in range(1, int(max_iter) + 1):
        if theta is not None:                                    # 1. filter: damp [lo, cut], the smallest Ritz value of the block
            cut, top = float(theta[-1]), float(theta[0])
            half, mid = max((cut - lo) / 2, 1e-30 * top), (cut + lo) / 2
            s1 = half / (top - mid)
            s = s1
            csr_cheb_step(plan, x, a=s / half, b=-mid * s / half, out=b1)
            old, cur = x, b1
            for _ in range(2, int(degree) + 1):
                s_next = 1.0 / (2.0 / s1 - s)
                csr_cheb_step(plan, cur, x=old, a=2 * s_next / half, b=-2 * s_next * mid / half, g=-s * s_next, out=old)
                old, cur, s = cur, old, s_next
            x, b1 = cur, old
        x.div_(torch.linalg.vector_norm(x, dim=0).clamp_min(1e-30))      # 2. orthonormalise: columns to unit norm, Cholesky-QR twice
        x, b1 = _cholesky_qr(x, b1)
        x, b1 = _cholesky_qr(x, b1)
        ax = csr_cheb_step(plan, x, out=b2)                       # 3. Rayleigh-Ritz
        h = torch.mm(x.t(), ax).double().cpu().numpy()
        w, q = np.linalg.eigh((h + h.T) / 2)
        theta, q = w[::-1].copy(), np.ascontiguousarray(q[:, ::-1])
        if not theta[0] > 0.0:
            raise native.SageError(f"eigen_top: largest Ritz value {theta[0]!r} is not positive")
        qf = torch.from_numpy(q).to(device=dev, dtype=torch.float32)
        xr = torch.mm(x, qf, out=b3)
        res = torch.mm(ax, qf, out=b1)                            # 4. residual columns A X - X theta
        res.addcmul_(xr, torch.from_numpy(theta).to(device=dev, dtype=torch.float32).unsqueeze(0), value=-1.0)
        worst = float(torch.linalg.vector_norm(res[:, :k], dim=0).max())
        if history is not None:
            history.append(worst)
        x, b1, b2, b3 = xr, x, ax, res
        if worst <= tol * theta[0]:
            return torch.from_numpy(theta[:k].copy()), _fix_signs(_round_once(x[:, :k])), it
    raise native.SageError(f"eigen_top: subspace iteration failed to converge within {int(max_iter)} iterations (largest residual "
                           f"{worst:.3e}, tol * theta_1 = {tol * theta[0]:.3e})")


def row_order_workspace_bytes(n):
    """Bytes of the workspace sage_row_order needs (host arithmetic; 0 = n out of range)."""
    return int(native.lib().sage_row_order_workspace_bytes(int(n)))


def row_order(nodes, n_dev=None, first_row=0, out=None, workspace=None):
    """int32 [n]: the canonical order of a layer's rows (sage_row_order) -- rows [0, first_row) as they are, then the live rows by
    ascending node id, dead rows (at or past *n_dev) last.  nodes: int32 [n] device tensor, the layer's node ids; n_dev: int32 [1]
    device tensor or None.  What embed_grad and the reproducible weight gradient sum in."""
    _need_gpu()
    _chk(nodes, torch.int32, "nodes", 1)
    n = nodes.shape[0]
    if n < 1:
        raise native.SageError("row_order: no rows")
    _opt_i32(n_dev, "n_dev", min_len=1)
    if out is None:
        out = torch.empty(n, dtype=torch.int32, device=nodes.device)
    _chk(out, torch.int32, "out", 1)
    if out.shape[0] < n:
        raise native.SageError(f"row_order: out has {out.shape[0]} entries for {n} rows")
    workspace = _workspace("row_order", row_order_workspace_bytes(n), workspace, nodes.device, f"n = {n}")
    native.check(native.lib().sage_row_order(native.ptr(nodes), n, native.ptr(n_dev), int(first_row), native.ptr(out), native.ptr(workspace),
                                             workspace.numel(), native.stream_handle()), "row_order")
    return out


def embed_grad_workspace_bytes(n, k, embed_rows, dim):
    """Bytes of the workspace sage_embed_grad needs (host arithmetic; 0 = shape out of range)."""
    return int(native.lib().sage_embed_grad_workspace_bytes(int(n), int(k), int(embed_rows), int(dim)))


def _embed_terms(who, grad_agg, nbr, cnt, n_dev, row_order):
    """What embed_grad and embed_grad_rows read: grad_agg [n, dim] over the sets (nbr, cnt), n_dev and row_order; returns (ldg, n, k, dim)."""
    _need_gpu()
    grad_agg, ldg = _row_major(grad_agg, "grad_agg")
    n, k = _sets(who, nbr, cnt, n_dev)
    if grad_agg.shape[0] < n:
        raise native.SageError(f"{who}: {n} sets, grad_agg has {grad_agg.shape[0]} rows, cnt {cnt.shape[0]} entries")
    _opt_i32(row_order, "row_order", 1, n)
    return ldg, n, k, grad_agg.shape[1]


def embed_grad(grad_agg, nbr, cnt, embed_rows, n_dev=None, row_order=None, out=None, workspace=None):
    """[embed_rows, dim]: the gradient of an embedding whose rows the sampled sets (nbr [n, k], cnt [n]) name, from the gradient of the
    sets' means grad_agg [n, dim]: row e is the sum of grad_agg[t] / c_t over the slots (t, j < c_t) with nbr[t, j] == e, the terms in
    `row_order` position (sage_embed_grad: 512-term chunks, fixed order, no atomics).  Stored, not accumulated: a row nobody names is
    zeros.  n_dev: int32 [1] live row count; row_order: int32 [n] from ops.row_order (None: rows as they lie); workspace: a uint8
    device tensor to reuse."""
    ldg, n, k, dim = _embed_terms("embed_grad", grad_agg, nbr, cnt, n_dev, row_order)
    rows = int(embed_rows)
    out, ld = _out_rows("embed_grad", out, rows, dim, grad_agg.device)
    if n == 0:                                             # the library launches nothing then: the zeros are written here
        out[:rows].zero_()
        return out
    workspace = _workspace("embed_grad", embed_grad_workspace_bytes(n, k, rows, dim), workspace, grad_agg.device,
                           f"n = {n}, k = {k}, embed_rows = {rows}, dim = {dim}")
    rc = native.lib().sage_embed_grad(native.ptr(grad_agg), ldg, dim, native.ptr(nbr), native.ptr(cnt), k, n, native.ptr(n_dev),
                                      native.ptr(row_order), native.ptr(out), rows, ld, native.ptr(workspace), workspace.numel(),
                                      native.stream_handle())
    native.check(rc, "embed_grad")
    return out


def embed_grad_rows_workspace_bytes(n, k, embed_rows, dim):
    """Bytes of the workspace sage_embed_grad_rows needs (host arithmetic; 0 = shape out of range; one value for every
    embed_rows >= n * k)."""
    return int(native.lib().sage_embed_grad_rows_workspace_bytes(int(n), int(k), int(embed_rows), int(dim)))


def embed_grad_rows(grad_agg, nbr, cnt, embed_rows, n_dev=None, row_order=None, max_rows=None, embed=None, lr=None, want_grad=True,
                    out=None, workspace=None):
    """embed_grad for the touched rows only, and / or their SGD update in place (sage_embed_grad_rows: nothing sized by embed_rows).
    -> (rows, num_rows, grad_rows): num_rows int32 [1] on the device, the number U of distinct embedding rows with a term; rows int32
    [max_rows], grad_rows [max_rows, dim]: the first min(U, max_rows) of them ascending and their sums, bit for bit the rows
    embed_grad stores (entries past that are left as they were); both None with want_grad=False.  max_rows: default min(n * k,
    embed_rows), which always holds every row.  embed [embed_rows, dim] with lr: embed[e] = fma(-lr, sum, embed[e]) for ALL U rows, in
    place, other rows untouched (torch's version counter of `embed` does not move: the caller's business).  out: (rows, num_rows,
    grad_rows) to write into (rows / grad_rows may be None there with want_grad=False); workspace: a uint8 device tensor to reuse."""
    who, P = "embed_grad_rows", native.ptr
    ldg, n, k, dim = _embed_terms(who, grad_agg, nbr, cnt, n_dev, row_order)
    rows, dev = int(embed_rows), grad_agg.device
    t = _touched_out(who, n, dim, rows, min(n * k, rows) if max_rows is None else int(max_rows), embed, "embed", lr, want_grad, out, dev)
    if n == 0:
        return t.result
    workspace = _workspace(who, embed_grad_rows_workspace_bytes(n, k, rows, dim), workspace, dev,
                           f"n = {n}, k = {k}, embed_rows = {rows}, dim = {dim}")
    rc = native.lib().sage_embed_grad_rows(P(grad_agg), ldg, dim, P(nbr), P(cnt), k, n, P(n_dev), P(row_order), rows, *t.args, P(workspace),
                                           workspace.numel(), native.stream_handle())
    native.check(rc, who)
    return t.result


def xent_head_supported(dim, num_classes):
    return bool(native.lib().sage_xent_head_supported(int(dim), int(num_classes)))


def xent_head_workspace_bytes(n, dim, num_classes):
    """Bytes of the workspace sage_xent_head needs (host arithmetic; 0 = shape out of range)."""
    return int(native.lib().sage_xent_head_workspace_bytes(int(n), int(dim), int(num_classes)))


def xent_head(emb, w_cls, labels=None, scale=None, scores=False, pred=False, grads=True, workspace=None, out=None):
    """model.py:59-69 + model.py:249: scores = emb . w_cls^T, CrossEntropyLoss and its gradients in one call (sage_xent_head).
    emb [n, dim], w_cls [C, dim] (the reference Parameter), labels int64 [n] or None (the inference form: scores / pred only).
    scale: factor of the summed loss, default 1 / n (a data-parallel shard passes 1 / global_batch).
    scores / pred / grads: which outputs to produce -- with labels the loss always is; grads = grad_emb and grad_w.
    out: dict of tensors to write into instead of fresh ones (keys as returned; rows beyond n are left alone).
    -> dict with the requested ones of scores [n, C], pred int32 [n], loss [1], grad_emb [n, dim], grad_w [C, dim]."""
    _need_gpu()
    emb, lde = _row_major(emb, "emb")
    w_cls, ldw = _row_major(w_cls, "w_cls")
    n, dim = emb.shape
    c = w_cls.shape[0]
    if w_cls.shape[1] != dim:
        raise native.SageError(f"xent_head: w_cls is {tuple(w_cls.shape)}, emb is {dim} wide")
    if n < 1:
        raise native.SageError("xent_head: no rows")
    if not xent_head_supported(dim, c):
        raise native.SageError(f"xent_head: no kernel for dim = {dim}, num_classes = {c}")
    if labels is None:
        if grads:
            raise native.SageError("xent_head: gradients need labels")
    else:
        _chk(labels, torch.int64, "labels", 1)
        if labels.shape[0] != n:
            raise native.SageError(f"xent_head: {labels.shape[0]} labels for {n} rows")
    dev = emb.device
    out = dict(out or {})
    res = {}

    def take(name, want, shape, dtype=torch.float32):
        if not want:
            return None
        t = out.get(name)
        if t is None:
            t = torch.empty(shape, dtype=dtype, device=dev)
        elif not t.is_cuda or t.dtype != dtype or t.dim() != len(shape) or t.shape[0] < shape[0] or tuple(t.shape[1:]) != tuple(shape[1:]):
            raise native.SageError(f"xent_head: out[{name!r}] is {tuple(t.shape)} {t.dtype}, expected {tuple(shape)} {dtype}")
        res[name] = t[:shape[0]]
        return res[name]

    t_scores = take("scores", scores, (n, c))
    t_pred = take("pred", pred, (n,), torch.int32)
    t_loss = take("loss", labels is not None, (1,))
    t_gemb = take("grad_emb", grads, (n, dim))
    t_gw = take("grad_w", grads, (c, dim))
    lds = ldg = ldgw = 0
    if t_scores is not None:
        t_scores, lds = _row_major(t_scores, "scores")
    if t_gemb is not None:
        t_gemb, ldg = _row_major(t_gemb, "grad_emb")
        t_gw, ldgw = _row_major(t_gw, "grad_w")
    if t_pred is not None:
        _chk(t_pred, torch.int32, "pred", 1)
    need = xent_head_workspace_bytes(n, dim, c)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    elif not _is_workspace(workspace, dev) or workspace.numel() < need:          # stricter than _workspace: a short one is refused
        raise native.SageError(f"xent_head: workspace must be a uint8 device tensor of >= {need} bytes")
    rc = native.lib().sage_xent_head(native.ptr(emb), lde, dim, native.ptr(w_cls), ldw, c, native.ptr(labels), n,
                                     float(1.0 / n if scale is None else scale), native.ptr(t_scores), lds, native.ptr(t_pred),
                                     native.ptr(t_loss), native.ptr(t_gemb), ldg, native.ptr(t_gw), ldgw, native.ptr(workspace),
                                     workspace.numel(), native.stream_handle())
    native.check(rc, "xent_head")
    return res
