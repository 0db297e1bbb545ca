"""TwoHopEngine: the 2-layer forward of graphsage/model.py:219-222 as ONE C call.

Everything the reference rebuilds per batch in Python (adjacency lookups, set
sampling, set union, id->column dict, dense mask) is device resident here:
CSR adjacency, the fp32 feature table and both weight matrices stay in HBM, and
`forward` enqueues sample -> frontier -> sample -> layer 1 -> layer 2 on the
current stream without a host round trip (sage_forward2, include/sage355.h).
"""
import ctypes
import os
from operator import attrgetter

import torch

from . import native
from .ops import ACT_RELU, _chk, _need_gpu, _row_major, as_ids, refuse_bf16


def pretransform_table(table, w1, rows_per_call=1 << 18):
    """INFERENCE at fixed weights, gcn encoder (encoders.py:56-61 with gcn=True): the mean is linear, so
    relu(W1 . mean(X[nbrs])) = relu(mean(Y[nbrs])) with Y = X . W1^T -- layer 1's contraction moves from every forward to weight-
    preparation time (once per weight update: 2 N D0 H1 flop, ~1 ms for a million 256-wide rows), the gather reads rows of H1 floats
    instead of D0 (half the bytes at 256 -> 128) and the per-batch contraction shrinks to H1 x H1.

        y, eye = pretransform_table(table, w1)                       # [N, H1] fp32 on the table's device, identity [H1, H1]
        eng = TwoHopEngine(rowptr, col, y, eye, w2, k1, k2)          # or RolePipeline(rowptr, col, y, eye, w2, ...)

    The engine is used UNCHANGED: with W1 := I the split-bf16 contraction returns its operand exactly (x = hi + mid + lo times 1.0); and
    since the returned identity is MARKED as such, the split layer skips that contraction altogether (the gather applies the activation
    and writes h1) -- the same bits, one launch and one round trip of the means less.
    Same sampled sets as the plain engine for the same keys; values equal to a few fp32 roundings (the sums are associated
    differently: mean of products instead of product of the mean) -- inside the 1e-5 parity bar, not bit-identical.  Differences by
    construction: non-finite FEATURES meet W1 before the mean (Inf - Inf cases of torch.mm land elsewhere); training needs the plain
    engine (Y is stale after every optimizer step; call this again after an update of W1).  Not for the concat encoder (two weight
    halves meet different rows there).  Y is computed by this library's own fp32-accurate contraction (sage_linear_act)."""
    from . import ops
    _need_gpu()
    if w1.dim() != 2 or table.dim() != 2 or w1.shape[1] != table.shape[1]:
        raise native.SageError(f"pretransform_table: W1 {tuple(w1.shape)} does not fit a {table.shape[1]}-wide table (gcn encoder only)")
    n, h1 = table.shape[0], w1.shape[0]
    w = w1.detach().to(table.device, torch.float32).contiguous()
    y = torch.empty((n, h1), dtype=torch.float32, device=table.device)
    for lo in range(0, n, rows_per_call):
        hi = min(n, lo + rows_per_call)
        ops.linear_act(table[lo:hi], w, act=ops.ACT_NONE, out=y[lo:hi])
    eye = torch.eye(h1, dtype=torch.float32, device=table.device)
    eye._sage_identity = True          # TwoHopEngine then declares it to the library (sage_model_t.w1_is_identity): layer 1's contraction is
    return y, eye                      # skipped and the column-sliced gather applies the activation and writes h1 itself


class _TableCopies:
    """The feature table as the kernels read it, one object per engine and its siblings and the only writer of: `src`, the caller's
    tensor; `table` / `ld`, the row-major working table -- `src` itself, or a private copy when the rows are renumbered (`degrees`:
    internal node i is the caller's node_order[i], descending degree, stable; new_of_old inverts it) or the 16-B-per-lane kernels
    cannot take `src` (width or leading dimension no multiple of 4 floats, base not 16-byte aligned: zero-padded, pads never
    written); `sliced`, the optional slice-major copy of `table`.  Each copy has ONE stamp, the version counter of what it was
    derived from, and is rewritten IN PLACE (role pipelines and captured graphs hold its address) on the current stream of the
    engine that notices: engines that share it on other streams must be ordered behind that by the caller (RolePipeline: join ->
    update -> fork).  Plain tensor work, on any device.

    Slice-major copy: float[d0 / W][N][W] (W = 32 floats = 128-byte slices by default) for the column-sliced layer-1 gather, so that
    the XCD that owns a slice reads ONE contiguous array -- consecutive hub rows' slices share DRAM pages and L2 sets -- instead of
    128 bytes out of every KiB.  Same-box A/B at config 3, gcn encoder: row-major 65.6 us per forward, slice-major 256-B slices
    62.8, 128-B slices + one destination row per lane group 60.6 (gather alone 42.5 -> 37.5 us); config 4 (2^23 nodes) 96.0 ->
    86.2; caller's node order 73.3 -> 61-64.  The concat encoder gets SLOWER with it (90 -> 96 us: its pacemaker is the two-pass
    contraction, which a more aggressive gather beside it slows down), so "auto" = gcn encoder only.  Costs a second copy of the
    table in HBM (1 GB of 288 at config 3); the row-major one stays for whole-row consumers (the concat encoder's own rows, the
    backward, read-back).  slice_major: "auto" / True / False; SAGE_TABLE_SLICED = 0: never, 1: "auto" as above, 2: "auto" includes
    the concat encoder (A/B); SAGE_TABLE_SLICE_FLOATS = 32 / 64 / 128 picks W.  Both are read once, here."""

    def __init__(self, table, ld, num_nodes, degrees=None, slice_major="auto", concat=False):
        self.src, self.d0 = table, table.shape[1]
        self.node_order = self.new_of_old = None
        if degrees is not None:
            self.node_order = torch.sort(degrees, descending=True, stable=True).indices
            self.new_of_old = torch.empty_like(self.node_order, dtype=torch.int32)
            self.new_of_old[self.node_order] = torch.arange(len(degrees), dtype=torch.int32, device=degrees.device)
        d0p = -(-self.d0 // 4) * 4
        if degrees is not None or d0p != self.d0 or ld % 4 != 0 or table.data_ptr() % 16 != 0:
            rows = len(degrees) if degrees is not None else table.shape[0]
            self.table, self.ld, self.version = torch.zeros((rows, d0p), dtype=torch.float32, device=table.device), d0p, None
            self.sync()
        else:
            self.table, self.ld, self.version = table, ld, table._version
        env = os.environ.get("SAGE_TABLE_SLICED", "1")
        w = self.slice_floats = int(os.environ.get("SAGE_TABLE_SLICE_FLOATS", "32"))
        # whole slices, at least two of them, of rows that lie back to back, one per node
        self.want_sliced = (slice_major is True or (slice_major == "auto" and (env == "2" or (not concat and env != "0")))) and (
            w in (32, 64, 128) and d0p % w == 0 and d0p >= 2 * w and self.ld == d0p and self.table.shape[0] == num_nodes)
        self.sliced = self.sliced_version = None

    def version_key(self):
        return self.src._version

    def sync(self, force=False):
        """Re-derive the private row-major copy from the caller's table when its version counter has moved since the last copy,
        or always (force).  An integer compare when nothing changed; a no-op when the working table IS the caller's."""
        if self.table is self.src or (not force and self.src._version == self.version):
            return
        with torch.no_grad():
            self.table[:, :self.d0].copy_(self.src if self.node_order is None else self.src[self.node_order])
        self.version = self.src._version

    def slice_major(self, force=False):
        """The slice-major copy (None: not wanted, or this shape has none): built at the first request, refreshed when the working
        table's version counter has moved since, or always (force).  Every requester gets the same tensor."""
        if self.want_sliced and (force or self.sliced_version != self.table._version):
            rows, w = self.table.shape[0], self.slice_floats
            with torch.no_grad():
                src = self.table.view(rows, -1, w).permute(1, 0, 2)
                if self.sliced is None:
                    self.sliced = src.contiguous()
                else:
                    self.sliced.copy_(src)
            self.sliced_version = self.table._version
        return self.sliced


class _WeightCopies:
    """The weight matrices as the kernels read them, one object per engine family: the caller's w1 [h1, m * d0] / w2 [h2, m * h1]
    themselves (m = 2 chunks for the concat encoder), or, when d0 or h1 is no multiple of 4 floats (Cora's 1433 raw features, the
    reference's default 50-wide layer 1, model.py:543), copies with every chunk and h1 zero-padded to one, rewritten in place when
    `version_key()` moves.  Zero weight rows / columns make the pad inert: relu(0) = 0, and sigmoid's 0.5 meets a zero column of W2.
    `epoch` is what invalidate() moves, for writes that the tensors' version counters do not see; the engines key their bf16
    planes with it too.  Same stream rule as _TableCopies."""

    def __init__(self, w1, w2, d0, concat=False):
        self.w1, self.w2, self.d0, self.h1, self.chunks = w1, w2, d0, w1.shape[0], 2 if concat else 1
        self.d0p, self.h1p = -(-d0 // 4) * 4, -(-self.h1 // 4) * 4
        self.padded = (self.d0p != d0) or (self.h1p != self.h1)
        self.epoch, self.w1p, self.w2p, self.key = 0, None, None, None

    def version_key(self):
        return (self.w1.data_ptr(), self.w1._version, self.w2.data_ptr(), self.w2._version, self.epoch)

    def invalidate(self):
        self.epoch += 1

    def tensors(self):
        if not self.padded:
            return self.w1, self.w2
        key = self.version_key()
        if key != self.key:
            m, d0, h1, d0p, h1p = self.chunks, self.d0, self.h1, self.d0p, self.h1p
            if self.w1p is None:
                self.w1p = torch.zeros((h1p, m * d0p), dtype=torch.float32, device=self.w1.device)
                self.w2p = torch.zeros((self.w2.shape[0], m * h1p), dtype=torch.float32, device=self.w1.device)
            with torch.no_grad():
                for c in range(m):
                    self.w1p[:h1, c * d0p: c * d0p + d0] = self.w1[:, c * d0: (c + 1) * d0]
                    self.w2p[:, c * h1p: c * h1p + h1] = self.w2[:, c * h1: (c + 1) * h1]
            self.key = key
        return self.w1p, self.w2p


class TwoHopEngine:
    def __init__(self, rowptr, col, table, w1, w2, k1, k2, concat=False, agg_self_loop=False, act1=ACT_RELU,
                 act2=ACT_RELU, nan_empty=True, fused=True, max_batch=4096, rowptr_outer=None, col_outer=None, relabel=None,
                 prepare_weights=True, slice_major="auto", embed_index=None, _parent=None):
        """rowptr/col: CSR of enc1.adj_lists (inner hop); rowptr_outer/col_outer: CSR of
        enc2.adj_lists when it differs (injected pre-sampled sets), default the same.
        w1 [h1, d0 | 2*d0], w2 [h2, h1 | 2*h1]: the Encoders' `weight` Parameters
        (referenced, not copied: an optimizer step is seen by the next forward).
        table: referenced too.  What the kernels read instead of the caller's tensors (renumbered / zero-padded / slice-major table
        copies, zero-padded weights) belongs to one _TableCopies and one _WeightCopies, built here and shared with siblings: re-derived
        in place whenever the caller's version counters move; refresh_table() / invalidate_weights() for writes that do not move them.
        embed_index (int32 [num_nodes], values in [0, R)): the featureless form (aggregators.py:68-71) -- `table` is then a trainable
        embedding [R, d0] with R <= num_nodes, node v reads row embed_index[v].  The engine translates the INNER column array once
        (col1 = embed_index[col]) and hands that to the library, so the sampled layer-1 sets hold embedding rows and every layer-1
        kernel runs unchanged on the R-row table; frontier, hash and outer hop keep node ids.  gcn encoder without the aggregator's
        self loop only, no relabel, d0 % 4 == 0, never a slice-major copy."""
        refuse_bf16(table, "TwoHopEngine")          # the sampled engine keeps private fp32 / bf16x3 copies: no bf16 table
        if embed_index is not None:          # before anything touches the device: every refusal is reachable without one
            slice_major = self._check_indexed(rowptr, table, embed_index, concat, agg_self_loop, relabel, slice_major, _parent)
        _need_gpu()
        self.rowptr1 = _chk(rowptr, torch.int64, "rowptr", 1)
        self.col1 = _chk(col, torch.int32, "col", 1)
        self.rowptr2 = self.rowptr1 if rowptr_outer is None else _chk(rowptr_outer, torch.int64, "rowptr_outer", 1)
        self.col2 = self.col1 if col_outer is None else _chk(col_outer, torch.int32, "col_outer", 1)
        if self.rowptr2.shape[0] != self.rowptr1.shape[0]:
            raise native.SageError("inner and outer CSR must cover the same node ids")
        table, ld = _row_major(table, "table")         # the caller's tensor itself (_row_major checks, never copies)
        if relabel not in (None, "degree"):
            raise native.SageError("relabel must be None or 'degree'")
        self.num_nodes = self.rowptr1.shape[0] - 1
        if embed_index is None and table.shape[0] < self.num_nodes:
            raise native.SageError(f"table has {table.shape[0]} rows for {self.num_nodes} nodes")
        self.d0, self.h1, self.h2 = table.shape[1], w1.shape[0], w2.shape[0]
        mult = 2 if concat else 1
        if tuple(w1.shape) != (self.h1, mult * self.d0) or tuple(w2.shape) != (self.h2, mult * self.h1):
            raise native.SageError(f"weight shapes {tuple(w1.shape)}, {tuple(w2.shape)} do not fit d0={self.d0}, concat={concat}")
        if _parent is not None:              # a sibling: the parent's owners themselves (sibling())
            self._tables, self._wcopies = _parent._tables, _parent._wcopies
        else:
            # relabel="degree": work on a copy of graph and table renumbered by descending degree, so that the rows gathered
            # most often are neighbours in memory (config 3: gather 46 -> 40 us).  The outer-hop kernel translates the seeds
            # (model.seed_map), so the caller keeps its ids and outputs stay in the caller's seed order; ids in intermediates()
            # are the INTERNAL ones (self.node_order[i] = caller's id of internal node i).
            # The device sampler is keyed by node id, so the sampled sets differ from the unrelabelled engine's (same law).
            deg = self.rowptr1[1:] - self.rowptr1[:-1] if relabel == "degree" else None
            self._tables = _TableCopies(table, ld, self.num_nodes, deg, slice_major, concat)
            if relabel == "degree":
                self._renumber_graph()
            self._wcopies = _WeightCopies(w1, w2, self.d0, concat)
        # what the model struct names as col1: the inner column array itself, or its translation into embedding rows (built once,
        # shared with siblings).  self.col1 / self.col2 stay node ids: the outer hop of a one-CSR engine keeps the untranslated array
        self.embed_index, self.embed_rows, self._col1_model = None, None, self.col1
        if embed_index is not None:
            self.embed_index, self.embed_rows = _chk(embed_index, torch.int32, "embed_index", 1), int(table.shape[0])
            if self._tables.table is not table:
                raise native.SageError("embed_index: the embedding must be readable in place (leading dimension a multiple of 4 floats, "
                                       "16-byte aligned): a private copy would go stale with every optimizer step")
            self._col1_model = _parent._col1_model if _parent is not None else self.embed_index[self.col1.long()].contiguous()
        self.d0p, self.h1p = self._wcopies.d0p, self._wcopies.h1p
        self._w1prep = self._w1prep_key = None
        self.prepare_weights = bool(prepare_weights)
        self.k1, self.k2 = int(k1), int(k2)
        self.concat, self.agg_self_loop = bool(concat), bool(agg_self_loop)
        self.act1, self.act2 = int(act1), int(act2)
        self.nan_empty, self.fused = bool(nan_empty), bool(fused)
        self.device = self.table.device
        self.max_batch, self.workspace, self.layout, self._last_batch, self._queue_batch = 0, None, native.WsLayout(), 0, 0
        self._model_key = self._model_c = self._model_q = None
        self._queue = self._cursor = self._graph = self._queue_seeds = self._graph_out = None      # set_queue / capture
        self.keep_means = False              # True: every forward leaves the layer-1 means in the workspace (training: backward_weights reads them)
        self._kept_means = False             # ... and whether the LAST forward did
        self.generation = 0                  # forwards run so far: a backward checks that the workspace still holds ITS forward
        self._bwd = None                     # scratch of backward_weights (allocated on first use)
        self._reserve(max_batch)

    # the owners' fields that callers read through the engine (bench.py, train.py, tests); read-only here
    table, table_ld = property(attrgetter("_tables.table")), property(attrgetter("_tables.ld"))
    node_order, _new_of_old = property(attrgetter("_tables.node_order")), property(attrgetter("_tables.new_of_old"))
    _table_sliced, _slice_floats = property(attrgetter("_tables.sliced")), property(attrgetter("_tables.slice_floats"))
    w1, w2, _padded = property(attrgetter("_wcopies.w1")), property(attrgetter("_wcopies.w2")), property(attrgetter("_wcopies.padded"))

    def _renumber_graph(self):
        """Both CSRs in the internal ids of relabel="degree" (the order itself is _TableCopies'), rows sorted."""
        n, order, new_of_old = self.num_nodes, self.node_order, self._new_of_old.long()

        def renumber(rowptr, col):
            d = rowptr[1:] - rowptr[:-1]
            src = new_of_old[torch.repeat_interleave(torch.arange(n, device=col.device), d)]
            key = torch.sort(src * n + new_of_old[col.long()]).values
            rp = torch.zeros(n + 1, dtype=torch.int64, device=col.device)
            rp[1:] = torch.cumsum(d[order], 0)
            return rp, (key % n).to(torch.int32)

        same = self.rowptr2 is self.rowptr1 and self.col2 is self.col1
        self.rowptr1, self.col1 = renumber(self.rowptr1, self.col1)
        self.rowptr2, self.col2 = (self.rowptr1, self.col1) if same else renumber(self.rowptr2, self.col2)

    @staticmethod
    def _check_indexed(rowptr, table, embed_index, concat, agg_self_loop, relabel, slice_major, parent):
        """The shapes an indexed engine takes (host checks on tensors of any device); -> the slice_major it runs with (False)."""
        if concat:
            raise native.SageError("embed_index: the concat encoder is not provided on an indexed engine: its own row would need a "
                                   "translated self_index (gcn encoder only)")
        if agg_self_loop:
            raise native.SageError("embed_index: the aggregator's self loop is not provided on an indexed engine: its set-union test "
                                   "compares node ids with what are embedding rows here")
        if relabel is not None:
            raise native.SageError("embed_index: relabel is not provided on an indexed engine: it renumbers the rows of a node table, and "
                                   "an embedding's rows are not nodes")
        if slice_major is True:
            raise native.SageError("embed_index: no slice-major copy on an indexed engine: its stride is num_nodes slices, the embedding "
                                   "has R rows and changes every step")
        if not isinstance(table, torch.Tensor) or table.dim() != 2 or not isinstance(rowptr, torch.Tensor) or rowptr.dim() != 1:
            raise native.SageError("embed_index: table must be the 2-d embedding [R, d0], rowptr the 1-d row pointer")
        rows, d0, num_nodes = table.shape[0], table.shape[1], rowptr.shape[0] - 1
        if d0 % 4 != 0:
            raise native.SageError(f"embed_index: embedding width {d0} is no multiple of 4: the kernels would read a zero-padded private "
                                   "copy, stale after every optimizer step")
        if rows < 1 or rows > num_nodes:
            raise native.SageError(f"embed_index: the embedding has R = {rows} rows for {num_nodes} nodes (1 <= R <= num_nodes)")
        if not isinstance(embed_index, torch.Tensor) or embed_index.dtype != torch.int32 or embed_index.dim() != 1 or \
                embed_index.shape[0] != num_nodes:
            raise native.SageError(f"embed_index: expected an int32 tensor [{num_nodes}] (one embedding row per node)")
        if parent is None and num_nodes > 0:            # once, at construction (one synchronisation)
            lo, hi = int(embed_index.min()), int(embed_index.max())
            if lo < 0 or hi >= rows:
                raise native.SageError(f"embed_index: value {lo if lo < 0 else hi} outside [0, R = {rows})")
        return False

    def sibling(self):
        """Another engine over the SAME device graph / table / weights (shared, not copied) with a workspace, bf16 weight planes and
        model struct of its own: what every additional mini-batch in flight needs.  It holds this engine's _TableCopies and
        _WeightCopies themselves: whichever engine notices an update re-derives the copies once, for all of them."""
        return TwoHopEngine(self.rowptr1, self.col1, self._tables.src, self.w1, self.w2, self.k1, self.k2, concat=self.concat,
                            agg_self_loop=self.agg_self_loop, act1=self.act1, act2=self.act2, nan_empty=self.nan_empty, fused=self.fused,
                            max_batch=self.max_batch, rowptr_outer=self.rowptr2, col_outer=self.col2, relabel=None,
                            prepare_weights=self.prepare_weights, slice_major=False if self.embed_index is not None else "auto",
                            embed_index=self.embed_index, _parent=self)

    def _weights(self):
        """The weight tensors the kernels read: the caller's own, or zero-padded copies kept in step with them."""
        return self._wcopies.tensors()

    def invalidate_weights(self):
        """The weights were written in a way that does not move their version counters (`.data`, a collective, a replayed hipGraph):
        move the weights epoch that the shared zero-padded copies and every engine's own bf16 planes are keyed with; the next forward
        of this engine or a sibling rebuilds what it reads, in place, from the tensors as they are NOW.  In-place writes that move the
        version counters (an optimizer step, `w.add_(...)` under no_grad) need no call: the next forward notices them.  Between
        replays of a captured graph use refresh_weights() instead."""
        self._wcopies.invalidate()
        self._model_key = None

    def refresh_weights(self):
        """Re-read the caller's weights NOW, whatever wrote them, into the zero-padded copies and the bf16 planes, in place: the call to
        make before replaying a captured graph after any weight update (a replay does not look at version counters)."""
        self.invalidate_weights()
        self._model(queued=self._queue is not None)

    def _prepare_w1(self, w1):
        """enc1.weight split into bf16 planes in the contraction kernel's register order (sage_prepare_weights), redone
        whenever the weight tensor, its version counter or the weights epoch changes; None when this layer shape has no prepared form."""
        L = native.lib()
        need = L.sage_prepared_weight_bytes(self.d0p, self.h1p, int(self.concat))
        if need == 0 or not self.prepare_weights:
            return None
        key = (w1.data_ptr(), w1._version, self._wcopies.epoch)
        if self._w1prep is None or self._w1prep.numel() != need:
            self._w1prep = torch.empty(need, dtype=torch.uint8, device=self.device)
            self._w1prep_key = None
        if self._w1prep_key != key:
            native.check(L.sage_prepare_weights(w1.data_ptr(), w1.stride(0), self.d0p, self.h1p, int(self.concat), self._w1prep.data_ptr(),
                                                need, torch.cuda.current_stream().cuda_stream), "prepare_weights")
            self._w1prep_key = key
        return self._w1prep

    def refresh_table(self):
        """The table was written in a way that does not move its version counter (`.data`, a collective, a replayed hipGraph): re-read
        it into the shared table copies (renumbered / zero-padded, and the slice-major one where it exists) in place, on the current
        stream: held pointers stay valid; siblings on other streams must be ordered behind this call.  In-place writes that move the
        version counter (`table[rows] = x`) need no call before a forward; before a REPLAY of a captured graph call this after any."""
        self._tables.sync(force=True)
        if self._tables.sliced is not None:
            self._tables.slice_major(force=True)

    def _wants_means(self):
        """Does this forward have to leave the layer-1 means in the workspace (sage_model_t.keep_means)?  Yes for an engine that trains
        (keep_means: EngineTrainer, autograd._TwoHop -- backward_weights reads them) and for any forward made under grad mode on weights
        that require a gradient; otherwise the library may run the split layer 1 as one launch that never writes them (same h1 bits)."""
        return bool(self.keep_means or (torch.is_grad_enabled() and (self.w1.requires_grad or self.w2.requires_grad)))

    def _model(self, queued=False, keep_means=False):
        """The C model struct over the copies as they are NOW (brought up to date here), rebuilt only when an address in it moved."""
        self._tables.sync()
        # layer 1 of THIS engine's layout decides whether its struct names the slice-major copy (no layout yet: not split)
        sliced = self._tables.slice_major() if self.layout.layer1_split else None
        w1, w2 = self._weights()
        prep = self._prepare_w1(w1.detach())
        key = (w1.data_ptr(), w2.data_ptr(), self._queue.data_ptr() if self._queue is not None else 0, prep.data_ptr() if prep is not None else 0,
               sliced.data_ptr() if sliced is not None else 0)
        if self._model_key != key:
            self._build_model(key, w1, w2, prep, sliced)
        m = self._model_q if queued else self._model_c
        m.keep_means = int(bool(keep_means))
        return m

    def _build_model(self, key, w1, w2, prep, sliced):
        _row_major(w1.detach(), "w1")
        _row_major(w2.detach(), "w2")
        if not (w1.is_contiguous() and w2.is_contiguous()):
            raise native.SageError("weights must be contiguous")
        self._model_c = native.Model(
            self.rowptr1.data_ptr(), self._col1_model.data_ptr(), self.rowptr2.data_ptr(), self.col2.data_ptr(), self.num_nodes,
            self.table.data_ptr(), self.table_ld, self.d0p, w1.data_ptr(), self.h1p, w2.data_ptr(), self.h2, self.k1, self.k2,
            int(self.concat), int(self.agg_self_loop), self.act1, self.act2, int(self.nan_empty), int(self.fused),
            int(self.max_batch))
        self._model_c.w1_prepared = prep.data_ptr() if prep is not None else None
        self._model_c.seed_map = self._new_of_old.data_ptr() if self._new_of_old is not None else None
        self._model_c.table_sliced = sliced.data_ptr() if sliced is not None else None
        self._model_c.table_slice_floats = self._slice_floats
        self._model_c.w1_is_identity = 1 if (getattr(self.w1, "_sage_identity", False) and not self.concat and not self._padded) else 0
        self._model_q = None
        if self._queue is not None:
            self._model_q = native.Model.from_buffer_copy(self._model_c)
            self._model_q.queue = self._queue.data_ptr()
            self._model_q.queue_len = self._queue.shape[0]
            self._model_q.queue_cursor = self._cursor.data_ptr()
        self._model_key = key

    # ---- device-side batch queue + hipGraph replay (no per-batch host work) ----
    def set_queue(self, seeds, rng_seeds):
        """seeds: int32 device tensor [S, B] (kept alive by the engine); rng_seeds: S sampler keys.
        Builds the ring of sage_batch_t descriptors the kernels read (include/sage355.h)."""
        if not (isinstance(seeds, torch.Tensor) and seeds.is_cuda and seeds.dtype == torch.int32 and seeds.dim() == 2
                and seeds.is_contiguous()):
            raise native.SageError("set_queue: seeds must be a contiguous int32 device tensor [S, B]")
        s, b = seeds.shape
        if len(rng_seeds) != s:
            raise native.SageError("set_queue: one sampler key per batch")
        if seeds.numel() and (int(seeds.min()) < 0 or int(seeds.max()) >= self.num_nodes):     # one sync, outside any timed loop
            raise native.SageError(f"set_queue: seed id outside [0, {self.num_nodes})")
        self._reserve(b)
        desc = torch.empty((s, 2), dtype=torch.int64)
        desc[:, 0] = seeds.data_ptr() + torch.arange(s, dtype=torch.int64) * (b * 4)
        keys = [int(x) & 0xFFFFFFFFFFFFFFFF for x in rng_seeds]
        desc[:, 1] = torch.tensor([k - (1 << 64) if k >= (1 << 63) else k for k in keys], dtype=torch.int64)
        self._queue_seeds = seeds
        self._queue = desc.to(self.device)
        self._cursor = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._queue_batch = b
        self._graph = None
        self._model_key = None

    def forward_queued(self, out):
        """One forward on the batch at the queue cursor (advances it).  Capturable."""
        L = native.lib()
        self._kept_means = self._wants_means()
        rc = L.sage_forward2(self._model(queued=True, keep_means=self._kept_means), self.workspace.data_ptr(), self.workspace.numel(), None,
                             self._queue_batch, 0, out.data_ptr(), out.stride(0), torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            native.check(rc, "forward2 (queued)")
        self._last_batch = self._queue_batch
        self.generation += 1
        return out

    def capture(self, out=None, batches=1):
        """Capture queued forwards into a hipGraph (torch.cuda.CUDAGraph); replay() then runs batch after batch with a
        single graph launch each.  batches > 1: one replay embeds that many consecutive batches of the ring into
        out[0..batches-1] -- for small batches (Pubmed's 256 seeds: 20 us of GPU work) the host's graph launch is
        otherwise the bottleneck."""
        if self._queue is None:
            raise native.SageError("capture: call set_queue first")
        batches = int(batches)
        shape = (self._queue_batch, self.h2) if batches == 1 else (batches, self._queue_batch, self.h2)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
        elif tuple(out.shape) != shape:
            raise native.SageError(f"capture: `out` must have shape {shape}")
        self._graph_out = out
        outs = [out] if batches == 1 else [out[j] for j in range(batches)]
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):          # warm-up outside capture (function attributes, lazy init)
            self.forward_queued(outs[0])
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for o in outs:
                self.forward_queued(o)
        self._graph = g
        self._cursor.zero_()
        torch.cuda.synchronize()
        return out

    def replay(self):
        self._graph.replay()
        return self._graph_out

    def rewind(self, position=0):
        self._cursor.fill_(int(position))

    def _reserve(self, batch):
        if batch <= self.max_batch:
            return
        self.max_batch = int(batch)
        self._model_key = None
        model = self._model()
        native.check(native.lib().sage_forward2_layout(model, self.max_batch, self.layout), "forward2_layout")
        self.workspace = torch.zeros(self.layout.total_bytes, dtype=torch.uint8, device=self.device)
        native.check(native.lib().sage_forward2_init(model, self.workspace.data_ptr(), self.workspace.numel(), self.max_batch,
                                                     torch.cuda.current_stream().cuda_stream), "forward2_init")
        self._graph = None

    def forward(self, seeds, seed=0, out=None, stage_events=None):
        """seeds: int32 device tensor (or anything as_ids takes) -> out [B, h2] on device.
        `seed` keys the sampler: the sets are a pure function of (seed, node id, hop).
        stage_events: optional (c_void_p * 8) of hipEvent_t recorded around the four stages."""
        if not (isinstance(seeds, torch.Tensor) and seeds.is_cuda and seeds.dtype == torch.int32 and seeds.is_contiguous()):
            seeds = as_ids(seeds, self.device, self.num_nodes)
        b = seeds.shape[0]
        if b > self.max_batch:
            self._reserve(b)
        if out is None:
            out = torch.empty((b, self.h2), dtype=torch.float32, device=self.device)
        elif out.shape != (b, self.h2) or out.dtype != torch.float32 or not out.is_cuda or out.stride(1) != 1:
            raise native.SageError("forward: `out` must be a [B, h2] fp32 device tensor with unit inner stride")
        L = native.lib()
        self._kept_means = self._wants_means()
        args = (self._model(keep_means=self._kept_means), self.workspace.data_ptr(), self.workspace.numel(), seeds.data_ptr(), b,
                int(seed) & 0xFFFFFFFFFFFFFFFF, out.data_ptr(), out.stride(0), torch.cuda.current_stream().cuda_stream)
        rc = L.sage_forward2(*args) if stage_events is None else L.sage_forward2_profiled(*args, stage_events)
        if rc != 0:
            try:
                native.check(rc, "forward2")
            finally:
                # a forward that stopped between two of its launches leaves sampled sets and frontier keys behind (layer 2's last
                # block is what cleans up): give the next call a clean workspace rather than a full hash table
                L.sage_forward2_init(args[0], self.workspace.data_ptr(), self.workspace.numel(), self.max_batch, args[-1])
        self._last_batch = b
        self.generation += 1
        return out

    # ---- backward of the last forward through the intermediates it left in the workspace (model.py:249) ----
    def backward_weights(self, out, grad_out, need_w1=True, need_embed=False, embed_lr=None):
        """Gradients of (w1, w2), in the caller's shapes, of the LAST forward on this engine: `out` is what it returned
        ([B, h2]), grad_out = d loss / d out.  Autograd of the reference's expression (mm / relu / cat / div) from
        the engine's own intermediates -- nbr / cnt / row2 / h1 (and the layer-1 means when layer 1 ran split) are still in the
        workspace, the layer-2 means are re-gathered -- with the C-ABI backward kernels.  The table is frozen (model.py:214-215):
        no gradient reaches it.  No host synchronisation: the frontier size never leaves the device.
        need_embed (an indexed engine only; a plain one raises): -> (g_w1, g_w2, g_embed), g_embed [R, d0] the dense gradient of the
        embedding, every row stored: g_h1 by the mean's backward over (row2, cnt2) -- (seed, slot) order -- then layer 1's grad_x on the
        kept means, then ops.embed_grad over (nbr1, cnt1) in ops.row_order's order of s1_nodes: no atomics, the bits do not depend
        on where the frontier's rows sit.  The weight gradients come from the same calls with or without it.
        need_embed="rows": -> (g_w1, g_w2, (rows, num_rows, grad_rows)), the gradient of the TOUCHED rows only (ops.embed_grad_rows):
        num_rows int32 [1] on the device, rows int32 [cap] ascending, grad_rows [cap, d0] the very bits need_embed=True stores in those
        rows, cap = min(max_s1 * k1, R); the buffers are the engine's, allocated on first use and rewritten by the next call.  With
        embed_lr=<float> the same call also applies embed[rows] = fma(-embed_lr, grad_rows, embed[rows]) to the engine's embedding.
        need_embed="update" (embed_lr required): the update alone, no gradient materialised; the third entry is num_rows.  Nothing on
        these two forms costs time or memory in proportion to R.  The update moves the embedding's version counter as an in-place
        torch op would, so a live RolePipeline over the same tensor orders its streams behind it at its next submit."""
        from . import ops
        if need_embed not in (False, True, "rows", "update"):
            raise native.SageError(f"backward_weights: need_embed = {need_embed!r}, expected False, True, 'rows' or 'update'")
        if embed_lr is not None and need_embed not in ("rows", "update"):
            raise native.SageError("backward_weights: embed_lr goes with need_embed='rows' or 'update'")
        if need_embed == "update" and embed_lr is None:
            raise native.SageError("backward_weights: need_embed='update' needs embed_lr")
        if need_embed and self.embed_index is None:
            raise native.SageError("backward_weights: need_embed on an engine without embed_index: its table is frozen features, "
                                   "no gradient reaches it")
        if getattr(self.w1, "_sage_identity", False):
            raise native.SageError("backward_weights: this engine serves a PRE-TRANSFORMED table (W1 is a declared identity): train with the "
                                   "plain engine on the raw features")
        lib = native.lib()
        st = native.stream_handle()
        P = native.ptr
        L, b = self.layout, self._last_batch
        dev = self.device
        if self._bwd is None or self._bwd["max_s1"] != L.max_s1:
            self._bwd = {"max_s1": L.max_s1, "nlive": torch.zeros(1, dtype=torch.int32, device=dev),
                         "agg1": None, "scratch": ops.Scratch(dev),
                         "any": torch.ones(1, dtype=torch.int32, device=dev)}
        sc = self._bwd
        first = b if self.concat else 0
        k2, h1p, d0p = self.k2, self.h1p, self.d0p
        # rows of layer 1 = first + frontier size, kept on the device (counters[8] is the read-back copy the forward's last block leaves)
        ws = self._ws_views()
        torch.add(ws("counters")[8:9], first, out=sc["nlive"])
        grad_out = grad_out.contiguous()
        w1p, w2p = self._weights()
        h1, row2, cnt2, nbr1, cnt1, s1_nodes = ws("h1"), ws("row2"), ws("cnt2"), ws("nbr1"), ws("cnt1"), ws("s1_nodes")
        self_row2 = ws("self_row2") if self.agg_self_loop else None
        scratch = sc["scratch"].get

        # ---- layer 2 backward: agg2 is recomputed (one small gather), then dW2 and d[h1_self | agg2].  The *_ws entry points are
        #      the reproducible forms (partial tiles added in a fixed order; inverted index instead of atomics): two runs of one
        #      schedule give the same bits, and a captured step equals the eager one bit for bit
        agg2 = ops.gather_mean(h1, row2, cnt2, self_row=self_row2, any_nonempty=sc["any"])
        mult = 2 if self.concat else 1
        g_w2p, g_x2 = ops.linear_act_backward(agg2, w2p, self.act2, out, grad_out, self_tab=h1 if self.concat else None,
                                              need_x=bool(need_w1 or need_embed),
                                              workspace=scratch("ws_dw2", ops.linear_act_backward_workspace_bytes(b, h1p, self.concat, self.h2)))
        g_w1p = None
        if need_w1 or need_embed:
            # ---- layer 1 backward: only dW1 (the table is frozen), summed over the OUTER EDGES (sage_two_hop_grad_w1): the terms
            #      act1'(h1[t]) . g_agg2[r] / c_r (x) X1[t] come in (seed, slot) order, so neither grad_h1 (a scatter) nor an order of the
            #      frontier's arbitrarily placed rows is needed, and the bits do not depend on the layout.  agg1 from the workspace
            #      (split layer) or recomputed on the live rows
            self_row1 = s1_nodes if self.agg_self_loop else None
            if L.layer1_split and self._kept_means:
                # the split layer (sliced gather + contraction) left the means of this very forward in the workspace: no second gather
                agg1 = ws("agg1")
            else:
                if sc["agg1"] is None:
                    sc["agg1"] = torch.zeros(L.max_s1, d0p, device=dev)
                ops.gather_mean(self.table, nbr1, cnt1, self_row=self_row1, any_nonempty=sc["any"], n_dev=sc["nlive"], out=sc["agg1"])
                agg1 = sc["agg1"]
        if need_w1:
            g_w1p = torch.zeros_like(w1p)
            ws1 = scratch("ws_dw1", lib.sage_two_hop_grad_w1_workspace_bytes(b, k2, d0p, int(self.concat), h1p))
            native.check(lib.sage_two_hop_grad_w1(P(g_x2), g_x2.stride(0), P(row2), P(cnt2), k2, P(self_row2), b, P(h1), h1p, h1p, self.act1,
                                                  P(agg1), agg1.stride(0), d0p, int(self.concat), P(self.table) if self.concat else None,
                                                  self.table_ld, P(s1_nodes) if self.concat else None, P(g_w1p), g_w1p.stride(0),
                                                  P(ws1), ws1.numel(), st), "two_hop_grad_w1")
        # padded widths (Cora 1433 -> 1436, 50 -> 52): gradients of the caller's own shapes
        if self._padded:
            g_w1 = None if g_w1p is None else torch.cat([g_w1p[:self.h1, c * d0p: c * d0p + self.d0] for c in range(mult)], 1)
            g_w2 = torch.cat([g_w2p[:, c * h1p: c * h1p + self.h1] for c in range(mult)], 1)
        else:
            g_w1, g_w2 = g_w1p, g_w2p
        if not need_embed:
            return g_w1, g_w2
        # ---- the embedding's gradient (indexed engine: gcn encoder, no self loop, d0p == d0): every step an existing entry point but the last
        n1, k1, rows = L.max_s1, self.k1, self.embed_rows
        if sc.get("g_h1") is None:
            sc["g_h1"] = torch.empty(n1, h1p, device=dev)
            sc["order"] = torch.empty(n1, dtype=torch.int32, device=dev)
        g_h1, order = sc["g_h1"], sc["order"]
        # 1. d loss / d h1: the layer-2 mean's backward over the outer samples, terms in (seed, slot) order; rows [0, nlive) are stored
        wsg = scratch("ws_gh1", lib.sage_gather_mean_backward_workspace_bytes(b, k2, n1))
        native.check(lib.sage_gather_mean_backward_ws(P(g_x2), g_x2.stride(0), h1p, P(row2), P(cnt2), k2, b, None, None, None, P(g_h1), n1,
                                                      P(sc["nlive"]), h1p, P(wsg), wsg.numel(), st), "gather_mean_backward_ws (layer 2)")
        # 2. d loss / d layer-1 means: layer 1's grad_x on the kept means (per row: no order to fix, and without a weight gradient
        #    the entry point takes no workspace)
        _, g_agg1 = ops.linear_act_backward(agg1, w1p, self.act1, h1, g_h1, n_dev=sc["nlive"], need_w=False)
        # 3. the frontier's rows by ascending node id, 4. the chunked sum over the sampled sets, which hold embedding rows
        ops.row_order(s1_nodes, n_dev=sc["nlive"], out=order, workspace=scratch("ws_order", ops.row_order_workspace_bytes(n1)))
        if need_embed not in ("rows", "update"):
            g_embed = ops.embed_grad(g_agg1, nbr1, cnt1, rows, n_dev=sc["nlive"], row_order=order, out=torch.empty(rows, d0p, device=dev),
                                     workspace=scratch("ws_embed", ops.embed_grad_workspace_bytes(n1, k1, rows, d0p)))
            return g_w1, g_w2, g_embed
        # the touched rows only: the compact gradient and / or the update of the embedding in place, nothing sized by R
        cap = min(n1 * k1, rows)
        if sc.get("num_rows") is None:
            sc["num_rows"] = torch.zeros(1, dtype=torch.int32, device=dev)
        rows_t = grad_t = None
        if need_embed == "rows":
            if sc.get("rows") is None:
                sc["rows"] = torch.empty(cap, dtype=torch.int32, device=dev)
                sc["grad_rows"] = torch.empty(cap, d0p, device=dev)
            rows_t, grad_t = sc["rows"], sc["grad_rows"]
        embed = self.table if embed_lr is not None else None                # the caller's tensor itself (an indexed engine reads it in place)
        ops.embed_grad_rows(g_agg1, nbr1, cnt1, rows, n_dev=sc["nlive"], row_order=order, max_rows=cap, embed=embed, lr=embed_lr,
                            want_grad=need_embed == "rows", out=(rows_t, sc["num_rows"], grad_t),
                            workspace=scratch("ws_embed_rows", ops.embed_grad_rows_workspace_bytes(n1, k1, rows, d0p)))
        if embed is not None:
            # the write went past torch: move the version counter as `embed.add_()` would, for everything keyed on it (RolePipeline's
            # _weights_key: join, fork behind this stream).  The engine itself holds no copy of an indexed table to refresh
            torch.autograd.graph.increment_version(self._tables.src)
        if need_embed == "rows":
            return g_w1, g_w2, (rows_t, sc["num_rows"], grad_t)
        return g_w1, g_w2, sc["num_rows"]

    # ---- read-back of the last forward's intermediates (tests, parity gate, byte counting) ----
    def _view(self, off, count, dtype):
        itemsize = torch.empty(0, dtype=dtype).element_size()
        return self.workspace[off: off + count * itemsize].view(dtype)

    def _ws_views(self):
        """field -> typed view of that field of the workspace, for the LAST forward's batch: the one table of layout field -> dtype,
        shape that backward_weights() and intermediates() read the workspace through."""
        L, b, i32, f32 = self.layout, self._last_batch, torch.int32, torch.float32
        fields = {"counters": (i32, (16,)), "s1_nodes": (i32, (L.max_s1,)), "nbr2": (i32, (b, self.k2)), "cnt2": (i32, (b,)),
                  "row2": (i32, (b, self.k2)), "self_row2": (i32, (b,)), "nbr1": (i32, (L.max_s1, self.k1)), "cnt1": (i32, (L.max_s1,)),
                  "h1": (f32, (L.max_s1, self.h1p)), "agg1": (f32, (L.max_s1, self.d0p))}

        def view(field):
            dtype, shape = fields[field]
            return self._view(getattr(L, field), torch.Size(shape).numel(), dtype).view(shape)
        return view

    def intermediates(self):
        """Sampled sets and layer-1 state of the LAST forward (synchronises).  On an indexed engine (embed_index) "nbr1" holds EMBEDDING
        rows, embed_index of the sampled node ids, since the inner column array is translated; every other id is a node id."""
        ws = self._ws_views()
        torch.cuda.synchronize()
        first = self._last_batch if self.concat else 0
        n1 = first + int(ws("counters").cpu()[8])          # [8..15]: the counters as the last forward left them
        return {
            "n_s1": n1, "first_frontier_row": first, "s1_nodes": ws("s1_nodes")[:n1],
            "nbr2": ws("nbr2"), "cnt2": ws("cnt2"), "row2": ws("row2"), "nbr1": ws("nbr1")[:n1], "cnt1": ws("cnt1")[:n1],
            "h1": ws("h1")[:n1, :self.h1],
            # the layer-1 means: only a split layer 1 writes them, and only when the forward was asked to keep them (keep_means)
            "agg1": ws("agg1")[:n1, :self.d0] if (self.layout.layer1_split and self._kept_means) else None,
        }


_PROCESS_ROLE_STREAMS = {}          # (device, distinct role letters, priorities) -> the role streams of the process's first such pipeline


class RolePipeline:
    """Consecutive 2-hop forwards software-pipelined over ROLE STREAMS (sage_pipe_*, include/sage355.h).

    Stage S (outer + inner sample), G (layer-1 gather), D (layer-1 contraction) and L (layer 2) each get a HIP
    stream; batch b+1 is gathered while batch b is contracted and batch b+2 is sampled, over `depth` workspaces.
    Bit-identical to TwoHopEngine.forward on the same (seeds, key).  `roles` maps the four roles onto streams:
    "SGDL" = four streams, "SGDD" = D and L share one, "SSSS" = one stream (= sage_forward2's launch order).
    `priorities`: per distinct stream, 0 = default, -1 = high (HIP stream priority); none named and four streams: S and L, the
    latency-bound roles, are high.  While stage D is empty (the one-launch layer 1) and stream L outranks streams G and D, the native
    pipe puts every odd batch's layer 1 on stream D's idle queue (`alternate_count`; SAGE_PIPE_G_ALT=0 / 1 forces it off / on), and
    every batch's inner sampler in front of its layer 1 (`inner_with_layer1_count`; SAGE_PIPE_SI_WITH_L1=0 / 1).
    The reference has no counterpart (model.py:240-252 is one batch at a time on the host)."""
    _h = None          # the native pipe; a class default because __del__ also meets a pipe whose __init__ failed or never ran

    def __init__(self, rowptr, col, table, w1, w2, k1, k2, batch, depth=4, roles="SGDL", priorities=None, streams=None, threads=None,
                 window=None, **engine_kwargs):
        self._broken, self._cap_stream = False, None
        refuse_bf16(table, "RolePipeline")
        if depth < 1 or depth > native.PIPE_MAX_DEPTH:
            raise native.SageError(f"RolePipeline: depth must be in [1, {native.PIPE_MAX_DEPTH}]")
        if len(roles) != 4:
            raise native.SageError("RolePipeline: roles is a 4-letter map of S, G, D, L onto streams, e.g. 'SGDL' or 'SGDD'")
        e0 = TwoHopEngine(rowptr, col, table, w1, w2, k1, k2, max_batch=batch, **engine_kwargs)
        self.engines = [e0] + [e0.sibling() for _ in range(depth - 1)]
        self.device, self.batch, self.depth, self.h2 = e0.device, int(batch), int(depth), e0.h2
        names = []
        for ch in roles:
            if ch not in names:
                names.append(ch)
        # No priorities named: with four role streams the latency-bound roles S and L get HIP's high priority.  That is what lets the
        # native pipe alternate layer 1 over streams G and D while stage D is empty (csrc/sage_pipe.hip, sage_pipe_alternate_count: it
        # does so where stream L outranks both); name priorities, e.g. {"L": 0}, to have others
        priorities = dict(priorities or ({"S": -1, "L": -1} if len(names) == 4 else {}))
        # stream D then carries every odd batch's layer 1, so a priority asked for role G has to reach both of layer 1's streams; a
        # priority named for D itself stands
        if os.environ.get("SAGE_PIPE_G_ALT", "") != "0" and len(names) == 4 and "G" in priorities and "D" not in priorities:
            priorities["D"] = priorities["G"]
        # Which hardware queue a NEW HIP stream lands on is the runtime's choice, and two role streams on one queue serialise (82-105 us per
        # forward instead of 59-90, seen for the second pipeline of a process).  So every pipeline of a process runs on the role streams
        # of the FIRST one with the same (device, role map, priorities) unless the caller hands in streams of its own or asks for new
        # ones (streams="new"); pipes that share streams and are used at the same time interleave in stream order, which is still correct.
        key = (str(self.device), "".join(names), tuple(int(priorities.get(ch, 0)) for ch in names))
        if streams is None and key in _PROCESS_ROLE_STREAMS:
            streams = _PROCESS_ROLE_STREAMS[key]
        if streams is not None and not isinstance(streams, str):
            if len(streams) != len(names):
                raise native.SageError(f"RolePipeline: {len(names)} distinct role streams needed, {len(streams)} given")
            self._streams = dict(zip(names, streams))
        else:
            self._streams = {ch: torch.cuda.Stream(device=self.device, priority=int(priorities.get(ch, 0))) for ch in names}
            _PROCESS_ROLE_STREAMS.setdefault(key, list(self._streams.values()))
        self.role_streams = [self._streams[ch] for ch in roles]
        ws = (ctypes.c_void_p * depth)(*[e.workspace.data_ptr() for e in self.engines])
        st = (ctypes.c_void_p * 4)(*[s.cuda_stream for s in self.role_streams])
        self._h = ctypes.c_void_p()
        native.check(native.lib().sage_pipe_create(e0._model(), self.batch, depth, ws, e0.workspace.numel(), st, ctypes.byref(self._h)),
                     "pipe_create")
        self._wkey = self._weights_key()
        self._keep = []
        # host enqueue threads (one per role stream; sage_pipe_set_threads): submit() then only posts the batch.  Opt-in (threads=True or
        # SAGE_PIPE_THREADS=1), because a caller that synchronises the device itself must then flush() first; bench.py opts in
        if threads is None:
            threads = os.environ.get("SAGE_PIPE_THREADS", "0") == "1" and len(names) == 4
        if window is None:
            window = int(os.environ.get("SAGE_PIPE_WINDOW", "0"))
        self.threads, self._window = False, int(window)
        if threads:
            self.set_threads(True, window)
        # the workspaces were zeroed and initialised, the slice-major table copy and the weight planes written, on the CURRENT stream; the
        # role streams are non-blocking streams of their own and would otherwise start the first batches beside that work (a sampler
        # filling a frontier table that a memset is still wiping leaves stale keys behind for good)
        self.fork()

    def set_threads(self, on, window=None):
        """Start (or drain and stop) the four host enqueue threads.  `window` > 0: role S enqueues batch b only once batch
        b - window has left the GPU (bounds the host's run-ahead); None keeps the pipe's setting."""
        if window is not None:
            self._window = int(window)
        native.check(native.lib().sage_pipe_set_threads(self._h, 1 if on else 0, self._window), "pipe_set_threads")
        self.threads = bool(on)

    def flush(self):
        """Every submitted batch has been ENQUEUED on the role streams (host enqueue threads; a no-op without them).  Call it
        before synchronising the device or the role streams yourself; join() / synchronize() do."""
        self._check(native.lib().sage_pipe_flush(self._h), "pipe_flush")

    def _check(self, rc, what):
        if rc != 0:
            self._broken = rc == native.ELAUNCH      # argument errors are raised before anything is enqueued: the pipe stays usable
            native.check(rc, what)

    def _check_usable(self):
        # a submit that failed between two of its enqueues leaves a batch half-way through the role streams, its workspace dirty and
        # its hand-off events unrecorded: later batches on that slot would wait for ever or sample into a full frontier table
        if self._broken:
            raise native.SageError("RolePipeline: an earlier submit failed half-way; synchronise, drop this pipe and create a new one")

    def _weights_key(self):
        """The CALLER's tensors' version counters (not those of the engine's private copies, which only move once they are rebuilt) and
        the weights epoch: integers, no side effects -- nothing is rewritten before the pipe has been joined."""
        e0 = self.engines[0]
        return e0._wcopies.version_key(), e0._tables.version_key()

    def _sync_weights(self):
        """Weights or table written in place since the last submit (version counters): re-prepare the weight planes / re-derive the
        private table copies on the CURRENT stream -- the stream such a write was made on -- and make the role streams wait for it."""
        key = self._weights_key()
        if key != self._wkey:
            self.join()                           # batches still in the pipe read the planes / the copies that are about to be rewritten
            m = self.engines[0]._model()          # re-pads / re-prepares the weights, re-derives the table copies in place: current stream
            native.check(native.lib().sage_pipe_update_weights(self._h, m.w1, m.w2, m.w1_prepared), "pipe_update_weights")
            self.fork()                           # the role streams wait for that
            self._wkey = key

    def refresh_table(self):
        """The table was written without moving its version counter (`.data`, a collective): re-read it into the engines' private
        copies in place and order the role streams behind that (and behind whatever wrote the table on the current stream).  Also the
        call to make before replaying a graph from capture() after any table write."""
        self.join()
        self.engines[0].refresh_table()
        self.fork()

    def refresh_weights(self):
        """The weights were written without moving their version counters (`.data`, a collective), or a graph from capture() is to be
        replayed after any weight update: re-pad / re-prepare them now, in place, with the role streams ordered behind that."""
        self.engines[0].invalidate_weights()      # moves the weights epoch, which is part of the key
        self._sync_weights()

    def __del__(self):
        if self._h:
            try:
                native.lib().sage_pipe_flush(self._h)
                torch.cuda.synchronize()
                native.lib().sage_pipe_destroy(self._h)
            except Exception:
                pass
            self._h = None

    def distinct_streams(self):
        """The pipe's distinct role streams, in first-use order of `roles` (pass them to another pipe's `streams=`)."""
        return list(self._streams.values())

    @property
    def express_count(self):
        """Batches of this pipe that found it idle and were enqueued whole on stream L (csrc/sage_pipe.hip, "express lane")."""
        return int(native.lib().sage_pipe_express_count(self._h))

    @property
    def alternate_count(self):
        """Batches of this pipe whose layer 1 was enqueued on stream D's idle queue (csrc/sage_pipe.hip, SAGE_PIPE_G_ALT=1)."""
        return int(native.lib().sage_pipe_alternate_count(self._h))

    @property
    def inner_with_layer1_count(self):
        """Batches of this pipe whose inner sampler was enqueued in front of their layer 1, on that launch's stream (csrc/sage_pipe.hip,
        SAGE_PIPE_SI_WITH_L1)."""
        return int(native.lib().sage_pipe_inner_with_layer1_count(self._h))

    def fork(self, stream=None):
        """Every role stream waits for `stream` (default: the current one): inputs written there are ready."""
        s = stream or torch.cuda.current_stream()
        native.check(native.lib().sage_pipe_fork(self._h, s.cuda_stream), "pipe_fork")

    def join(self, stream=None):
        """`stream` (default: the current one) waits for everything submitted so far."""
        s = stream or torch.cuda.current_stream()
        native.check(native.lib().sage_pipe_join(self._h, s.cuda_stream), "pipe_join")

    def submit_profiled(self, seeds, key, out, gather_events):
        """submit() with two hipEvent_t (a ctypes c_void_p * 2) recorded on stream G around the layer-1 gather."""
        self._sync_weights()
        self._check_usable()
        self._check(native.lib().sage_pipe_submit_profiled(self._h, seeds.data_ptr(), int(key) & 0xFFFFFFFFFFFFFFFF, out.data_ptr(),
                                                           out.stride(0), gather_events), "pipe_submit_profiled")

    def submit(self, seeds, key, out):
        """One batch: seeds int32 [batch] device tensor, out [batch, h2] fp32 device tensor (both must stay alive
        and unmodified until the batch has left the pipe: join() + synchronize, or an event on stream L)."""
        if not (isinstance(seeds, torch.Tensor) and seeds.is_cuda and seeds.dtype == torch.int32 and seeds.is_contiguous()
                and seeds.numel() == self.batch):
            raise native.SageError("RolePipeline.submit: seeds must be a contiguous int32 device tensor of `batch` ids")
        if out.shape != (self.batch, self.h2) or out.dtype != torch.float32 or not out.is_cuda or out.stride(1) != 1:
            raise native.SageError("RolePipeline.submit: `out` must be a [batch, h2] fp32 device tensor with unit inner stride")
        self._check_usable()
        self._sync_weights()
        self._check(native.lib().sage_pipe_submit(self._h, seeds.data_ptr(), int(key) & 0xFFFFFFFFFFFFFFFF, out.data_ptr(), out.stride(0)),
                    "pipe_submit")

    def submit_many(self, seeds, keys, out, segment_start=False):
        """seeds int32 [n, batch] (device, contiguous), keys: n sampler keys, out [slots, batch, h2] with slots >= depth
        (batch i lands in out[i % slots]) -- ONE host call enqueues all n batches."""
        if not (isinstance(seeds, torch.Tensor) and seeds.is_cuda and seeds.dtype == torch.int32 and seeds.is_contiguous()
                and seeds.dim() == 2 and seeds.shape[1] == self.batch):
            raise native.SageError("RolePipeline.submit_many: seeds must be a contiguous int32 device tensor [n, batch]")
        n = seeds.shape[0]
        if len(keys) != n:
            raise native.SageError("RolePipeline.submit_many: one sampler key per batch")
        if (out.dim() != 3 or out.shape[1:] != (self.batch, self.h2) or out.dtype != torch.float32 or not out.is_cuda
                or not out.is_contiguous() or out.shape[0] < self.depth):
            raise native.SageError("RolePipeline.submit_many: `out` must be a contiguous [slots >= depth, batch, h2] fp32 device tensor")
        self._sync_weights()
        karr = (ctypes.c_uint64 * n)(*[int(k) & 0xFFFFFFFFFFFFFFFF for k in keys])
        self._check_usable()
        self._check(native.lib().sage_pipe_submit_many(self._h, seeds.data_ptr(), self.batch, karr, n, out.data_ptr(), out.stride(1),
                                                       out.stride(0), out.shape[0], 1 if segment_start else 0), "pipe_submit_many")

    def reset(self):
        """Forget every submit (after synchronising): the next `depth` submits find their workspaces free."""
        native.check(native.lib().sage_pipe_reset(self._h), "pipe_reset")

    def capture(self, seeds, keys, out, stream=None):
        """The n batches seeds[i] / keys[i] -> out[i % slots] through the role streams, captured as ONE hipGraph:
        fork -> submit_many -> join on `stream` (default: a stream of the pipe's own).  -> (torch.cuda.CUDAGraph, stream);
        `graph.replay()` under `torch.cuda.stream(stream)` then runs all n batches with a single host call.  The graph embeds
        these seeds / keys / out tensors (keep them alive and unmodified in place of new data: write new seeds INTO `seeds`).
        Bit-identical to submit() on the same batches.  The pipe must be idle (synchronise first); eager submission afterwards
        needs reset()."""
        self._sync_weights()
        self._check_usable()
        if stream is None:
            stream = self._cap_stream = self._cap_stream or torch.cuda.Stream(device=self.device)
        self.flush()
        torch.cuda.synchronize()
        was_threaded = self.threads
        if was_threaded:
            self.set_threads(False)          # a capture records the calls of the capturing thread
        self.reset()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(stream):
            with torch.cuda.graph(g, stream=stream):
                self.fork(stream)
                self.submit_many(seeds, keys, out, segment_start=True)
                self.join(stream)
        self.reset()
        if was_threaded:
            self.set_threads(True)
        self._keep.append((seeds, out))
        return g, stream

    def synchronize(self):
        self.flush()
        for s in self._streams.values():
            s.synchronize()
