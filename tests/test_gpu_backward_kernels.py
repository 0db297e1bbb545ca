"""The backward kernels (csrc/sage_backward.hip, csrc/sage_backward_det.hip), called through the C ABI, against fp64.

Every reference is built here from the documented formula (include/sage355.h, "Backward of the two operators" onwards), in fp64
from the fp32 inputs the kernel saw.  Tolerance, elementwise: |got - want| <= 1e-5 * A, A the fp64 sum of the absolute values
of the terms (|dZ|^T |X| for a weight gradient, |dZ| |W| for grad_x, sum |g_r| / c_r for a table row); where A is 0 the output
is exactly 0.  An accumulated output (grad_weight, grad_w1) starts from a random G0 and got - G0 is checked; the one rounding of
the final "+=" is allowed for, and elements with A == 0 must keep G0's bits.  Also max |err| / max |want| <= 2e-5.  What the
header says is not written (rows past n_dev, padding columns, table rows past *table_rows_dev) is prefilled with a sentinel
and must keep it; input rows that must not be read hold NaN.

Paths (sage_backward.hip: linear_act_backward_impl):
    grad_x       bwd_dx_direct_kernel        out_dim % 4 == 0, ldg / ldo % 4 == 0, grad_out / out 16-byte aligned
                 bwd_gemm_kernel<0>          otherwise
    grad_weight  bwd_dw_direct_kernel<F|T>   _ws, even widths and lds, 8-byte aligned (T: concat with self_index)
                 bwd_gemm_kernel<1> partials _ws otherwise;  both followed by dw_reduce_kernel
                 bwd_gemm_kernel<1> atomics  legacy entry point
The launch tunables SAGE_BWD_DIRECT_BLOCKS and SAGE_BWD_BLOCKS are read once per process: other settings run in child
processes (test_backward_kernels_behind_the_launch_tunables).
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from sage355 import native

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND, MAXREL = 1e-5, 2e-5
SENTINEL = -31.5
RELU, SIGMOID, NONE = native.ACT_RELU, native.ACT_SIGMOID, native.ACT_NONE
ACT = {"relu": RELU, "sigmoid": SIGMOID, "none": NONE}
HALF_ULP = 2.0 ** -24
P = native.ptr


def _lib():
    return native.lib()


def _sync():
    torch.cuda.synchronize()


def _act_inputs(gen, rows, cols, act):
    """An `out` for the activation: relu with exact zeros, sigmoid in (0, 1), none anything."""
    if act == "relu":
        return torch.relu(torch.randn(rows, cols, generator=gen))
    if act == "sigmoid":
        return torch.rand(rows, cols, generator=gen) * 0.98 + 0.01
    return torch.randn(rows, cols, generator=gen)


def _act_grad64(y, act):
    """act'(pre) as the kernels compute it from the output y, fp64."""
    y = y.double()
    if act == "relu":
        return (y > 0).double()
    if act == "sigmoid":
        return y * (1 - y)
    return torch.ones_like(y)


def _view(big, rows, cols, shift=0):
    """rows x cols starting `shift` floats into the big array (ld = big's width)."""
    return big.view(-1)[shift:shift + big.shape[1] * (rows - 1) + cols].as_strided((rows, cols), (big.shape[1], 1)) \
        if rows > 0 else big[:0, :cols]


def _check(got, want, A, what, g0=None):
    """got (device) against want with the A bound; with g0 the output accumulated onto g0."""
    got = got.double().cpu()
    A = A.double()
    if g0 is not None:
        g0 = g0.double().cpu()
        zero = A == 0
        assert torch.equal(got[zero], g0[zero]), f"{what}: elements with no terms changed"
        delta = got - g0
        tol = BOUND * A + HALF_ULP * (g0 + want).abs() * 2
    else:
        zero = A == 0
        assert bool((got[zero] == 0).all()), f"{what}: elements with no terms are not 0"
        delta = got
        tol = BOUND * A
    err = (delta - want).abs()
    assert not bool(torch.isnan(delta).any()), f"{what}: NaN in the result"
    bad = err > tol
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements over the bound; worst {float((err - tol).max()):.3g}"
    scale = float(want.abs().max()) if want.numel() else 0.0
    if scale > 0:
        assert float(err.max()) / scale <= MAXREL, f"{what}: max relative error {float(err.max()) / scale:.3g}"


def _untouched(t, what):
    t = t.cpu()
    assert bool((t == SENTINEL).all()), f"{what}: written"


# ================================================================================ 1. linear_act backward
class Lin:
    """One linear_act_backward call: self_tab / agg / W / out / grad_out as views of wider arrays (ld = width + pad), based
    `shift` floats in.  mode: gcn, concat (self row r), idx (concat with self_index, a permutation into a taller table)."""

    def __init__(self, n, dim, out_dim, mode, act, pad=4, shift=0, seed=0):
        gen = torch.Generator().manual_seed(seed * 7919 + n + dim + out_dim)
        self.n, self.dim, self.out_dim, self.mode, self.act, self.pad, self.shift = n, dim, out_dim, mode, act, pad, shift
        self.ds = dim if mode != "gcn" else 0
        self.K = self.ds + dim
        rows = max(n, 1)
        self.agg_h = torch.randn(rows + 1, dim + pad, generator=gen)
        self.T = n + 50 if mode == "idx" else rows
        self.self_h = torch.randn(self.T + 1, dim + pad, generator=gen) if mode != "gcn" else None
        self.sidx = torch.randperm(self.T, generator=gen)[:n].to(torch.int32) if mode == "idx" else None
        self.w_h = torch.randn(out_dim + 1, self.K + pad, generator=gen) / np.sqrt(self.K)
        self.out_h = _act_inputs(gen, rows + 1, out_dim + pad, act)
        self.g_h = torch.randn(rows + 1, out_dim + pad, generator=gen)
        self.g0 = torch.randn(out_dim, self.K, generator=gen)

    # host views of the inputs (fp32)
    def _hv(self, big, cols):
        return _view(big, self.n, cols, self.shift)

    def reference(self, live):
        agg = self._hv(self.agg_h, self.dim)[:live].double()
        out = self._hv(self.out_h, self.out_dim)[:live]
        g = self._hv(self.g_h, self.out_dim)[:live].double()
        w = _view(self.w_h, self.out_dim, self.K, self.shift).double()
        dz = g * _act_grad64(out, self.act)
        if self.mode == "gcn":
            x = agg
        else:
            st = _view(self.self_h, self.T, self.dim, self.shift).double()
            x = torch.cat([st[self.sidx[:live].long()] if self.sidx is not None else st[:live], agg], 1)
        return dz.t() @ x, dz.abs().t() @ x.abs(), dz @ w, dz.abs() @ w.abs()

    def device_inputs(self, live):
        """Device copies; every input row past `live` holds NaN (and so does the self row only a dead row uses)."""
        def dev(big, rows, cols, dead_rows):
            h = big.clone()
            if len(dead_rows):
                _view(h, rows, cols, self.shift)[torch.tensor(dead_rows, dtype=torch.int64)] = float("nan")
            return h.to(DEV)
        dead = list(range(live, self.n))
        d = {"agg": dev(self.agg_h, self.n, self.dim, dead), "out": dev(self.out_h, self.n, self.out_dim, dead),
             "g": dev(self.g_h, self.n, self.out_dim, dead), "w": self.w_h.to(DEV)}
        if self.mode == "gcn":
            d["self"] = None
        else:
            d["self"] = dev(self.self_h, self.T, self.dim, [int(self.sidx[r]) for r in dead] if self.sidx is not None else dead)
        d["sidx"] = self.sidx.to(DEV) if self.sidx is not None else None
        return d

    def call(self, d, n_dev=None, ws=True, want_w=True, want_x=True, row_order=None, gw=None, gx=None, ldgw=None, ldgx=None):
        """Run the kernel; returns (grad_weight big, grad_x big) device arrays (or None)."""
        L = _lib()
        s = self.shift
        ldgw = ldgw or self.K + 3
        ldgx = ldgx or self.K + 5
        if want_w and gw is None:
            gw = torch.full((self.out_dim, ldgw), SENTINEL)
            gw[:, :self.K] = self.g0
            gw = gw.to(DEV)
        if want_x and gx is None:
            gx = torch.full((max(self.n, 1), ldgx), SENTINEL, device=DEV)
        def fp(big):
            return None if big is None else ctypes.c_void_p(big.data_ptr() + 4 * s)
        nd = None if n_dev is None else torch.tensor([n_dev], dtype=torch.int32, device=DEV)
        args = [fp(d["self"]), d["self"].shape[1] if d["self"] is not None else 0, P(d["sidx"]),
                fp(d["agg"]), d["agg"].shape[1], self.dim, fp(d["w"]), d["w"].shape[1], self.out_dim, ACT[self.act],
                fp(d["out"]), d["out"].shape[1], fp(d["g"]), d["g"].shape[1], self.n, P(nd),
                P(gw if want_w else None), ldgw, P(gx if want_x else None), ldgx]
        if ws:
            need = L.sage_linear_act_backward_workspace_bytes(self.n, self.dim, int(self.mode != "gcn"), self.out_dim)
            wsb = torch.empty(need, dtype=torch.uint8, device=DEV)
            native.check(L.sage_linear_act_backward_ws(*args, P(row_order), P(wsb), need, native.stream_handle()), "linear_act_backward_ws")
        else:
            native.check(L.sage_linear_act_backward(*args, native.stream_handle()), "linear_act_backward")
        _sync()
        return (gw if want_w else None), (gx if want_x else None)

    def verify(self, gw, gx, live, what):
        dw, dwA, dx, dxA = self.reference(live)
        if gw is not None:
            _check(gw[:, :self.K], dw, dwA, what + " grad_weight", g0=self.g0)
            _untouched(gw[:, self.K:], what + " grad_weight padding columns")
        if gx is not None:
            _check(gx[:live, :self.K], dx, dxA, what + " grad_x")
            _untouched(gx[:, self.K:], what + " grad_x padding columns")
            _untouched(gx[live:self.n], what + " grad_x rows past n_dev")


# (n, dim, out_dim, mode, act, pad, shift): the paths each row takes are in the comment (dW ws / dW legacy / dx)
LIN_CASES = [
    (1, 64, 4, "gcn", "relu", 4, 0),            # direct<false> / atomics / dx direct
    (2, 3, 12, "idx", "sigmoid", 1, 0),         # odd dim: gemm<1> partials / dx generic (ldo 13)
    (63, 50, 52, "concat", "none", 6, 0),       # direct<false> x2 / dx generic (ld 58 % 4 != 0)
    (64, 256, 128, "idx", "relu", 4, 0),        # direct<true> / dx direct
    (65, 258, 130, "gcn", "sigmoid", 4, 0),     # direct, grid.z = 2 / dx generic (out_dim % 4 != 0)
    (257, 1436, 256, "gcn", "relu", 8, 0),      # direct, grid.y = 6, grid.z = 2 / dx direct, 12 column blocks
    (257, 64, 2, "idx", "none", 4, 1),          # 4-byte shifted views: gemm<1> partials / dx generic
    (23000, 256, 128, "idx", "relu", 4, 0),     # many splits
    (23000, 50, 130, "gcn", "sigmoid", 2, 0),   # direct, out_dim > 128 / dx generic
    (2000, 3, 4, "concat", "relu", 3, 0),       # odd dim and ld: gemm<1> partials
    (300, 1, 12, "gcn", "none", 0, 0),          # dim 1
    (4000, 64, 256, "concat", "sigmoid", 4, 1), # shifted: gemm<1> partials with two M tiles / dx generic
    (63, 128, 52, "idx", "relu", 4, 1),         # shifted, self_index
    (129, 51, 7, "concat", "none", 0, 0),       # odd everything
]


def linear_checks(cases=LIN_CASES, legacy=True):
    for n, dim, out_dim, mode, act, pad, shift in cases:
        c = Lin(n, dim, out_dim, mode, act, pad, shift)
        for n_dev in (None, 0, n - 37, n + 5):
            if n_dev is not None and n_dev < 0:
                continue
            live = n if n_dev is None else max(0, min(n_dev, n))
            d = c.device_inputs(live)
            tag = f"n={n} dim={dim} out_dim={out_dim} {mode} {act} pad={pad} shift={shift} n_dev={n_dev}"
            gw, gx = c.call(d, n_dev)
            c.verify(gw, gx, live, tag + " _ws")
            if legacy:
                gw2, gx2 = c.call(d, n_dev, ws=False)
                c.verify(gw2, gx2, live, tag + " legacy")
                assert torch.equal(gx.view(torch.int32), gx2.view(torch.int32)), f"{tag}: grad_x differs between the entry points"
                gw3, _ = c.call(d, n_dev, want_x=False)
                assert torch.equal(gw3.view(torch.int32), gw.view(torch.int32)), f"{tag}: _ws grad_weight not reproducible"


@pytest.mark.parametrize("case", LIN_CASES, ids=lambda c: "n{}-d{}-o{}-{}-{}-p{}-s{}".format(*c))
def test_linear_act_backward_paths_match_fp64(case):
    linear_checks([case])


def test_linear_act_backward_null_outputs():
    """grad_x = NULL computes grad_weight alone; grad_weight = NULL needs no workspace and computes grad_x alone."""
    c = Lin(300, 64, 52, "idx", "relu")
    d = c.device_inputs(300)
    gw, _ = c.call(d, want_x=False)
    c.verify(gw, None, 300, "grad_x NULL")
    _, gx = c.call(d, want_w=False, ws=True)
    c.verify(None, gx, 300, "grad_weight NULL")
    L = _lib()
    # grad_weight NULL through _ws with no workspace at all
    gx2 = torch.full_like(gx, SENTINEL)
    s = d["self"]
    native.check(L.sage_linear_act_backward_ws(P(s), s.shape[1], P(d["sidx"]), P(d["agg"]), d["agg"].shape[1], 64, P(d["w"]),
                                               d["w"].shape[1], 52, RELU, P(d["out"]), d["out"].shape[1], P(d["g"]), d["g"].shape[1],
                                               300, None, None, 0, P(gx2), gx2.shape[1], None, None, 0, native.stream_handle()),
                 "linear_act_backward_ws without grad_weight")
    _sync()
    assert torch.equal(gx2.view(torch.int32), gx.view(torch.int32))


# ================================================================================ 2. row order
def _expected_order(nodes, n_dev, first):
    n = len(nodes)
    nn = n if n_dev is None else min(n_dev, n)
    r = np.arange(n, dtype=np.int64)
    key = np.where(r < first, r, first + np.maximum(nodes.astype(np.int64), 0))
    key = np.where(r < nn, np.minimum(key, 0x7FFFFFFE), 0x7FFFFFFF)
    return np.argsort(key, kind="stable").astype(np.int32)


def _row_order(nodes, n_dev, first, ws_bytes=None):
    L = _lib()
    n = len(nodes)
    need = L.sage_row_order_workspace_bytes(n)
    assert need > 0
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device=DEV)
    order = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    nd = None if n_dev is None else torch.tensor([n_dev], dtype=torch.int32, device=DEV)
    rc = L.sage_row_order(P(torch.from_numpy(nodes).to(DEV)), n, P(nd), first, P(order), P(ws),
                          need if ws_bytes is None else ws_bytes, native.stream_handle())
    _sync()
    return rc, order.cpu().numpy()


@pytest.mark.parametrize("n,first,n_dev", [(1, 0, None), (1, 1, 1), (5, 0, 0), (300, 17, None), (300, 300, 300), (300, 0, 300),
                                           (4097, 64, 3000), (4097, 4097, 0), (23000, 1024, 20000)])
def test_row_order_matches_numpy(n, first, n_dev):
    """Rows [0, first) in place, then the live frontier rows by ascending node id, dead rows last (stable: in row order)."""
    rs = np.random.default_rng(n + first)
    nodes = rs.permutation(10 * n + 10)[:n].astype(np.int32)
    if n - first >= 3:
        nodes[first:first + 2] = [2 ** 31 - 1, 2 ** 31 - 2]   # node ids near 2^31: the key clamp
        nodes[-1] = -5
    rc, got = _row_order(nodes, n_dev, first)
    native.check(rc, "row_order")
    assert np.array_equal(got, _expected_order(nodes, n_dev, first))
    assert np.array_equal(np.sort(got), np.arange(n))


def test_row_order_short_workspace_refuses_without_a_launch():
    L = _lib()
    nodes = np.arange(1000, dtype=np.int32)
    need = L.sage_row_order_workspace_bytes(1000)
    rc, got = _row_order(nodes, None, 0, ws_bytes=need - 1)
    assert rc == native.ENOSPACE and bool((got == -7).all())


def _layer_layouts(n, first, dead, seed):
    """A layer of n rows: first seed rows, then frontier rows with distinct node ids; the second layout shuffles the live
    frontier rows.  Returns (nodes_a, nodes_b, perm) with rows_b[i] = rows_a[perm[i]]."""
    rs = np.random.default_rng(seed)
    nodes = rs.permutation(20 * n)[:n].astype(np.int32)
    live = n - dead
    perm = np.arange(n)
    perm[first:live] = first + rs.permutation(live - first)
    return nodes, nodes[perm], perm


@pytest.mark.parametrize("n,dim,out_dim,mode,shift,dead", [(3000, 64, 128, "idx", 0, 0), (3000, 64, 128, "idx", 0, 333),
                                                           (2500, 50, 52, "concat", 0, 0), (2500, 51, 52, "gcn", 0, 100),
                                                           (2100, 64, 130, "idx", 1, 77), (700, 256, 256, "gcn", 0, 31)])
def test_weight_gradient_does_not_depend_on_the_row_layout(n, dim, out_dim, mode, shift, dead):
    """The same layer laid out twice (frontier rows shuffled), each summed in sage_row_order's order: equal bits."""
    first = 200 if mode != "gcn" else 0
    c = Lin(n, dim, out_dim, mode, "relu", pad=4, shift=shift, seed=3)
    nodes_a, nodes_b, perm = _layer_layouts(n, first, dead, seed=n)
    live = n - dead
    da = c.device_inputs(live)
    rc, order_a = _row_order(nodes_a, live if dead else None, first)
    native.check(rc, "row_order")
    gwa, _ = c.call(da, n_dev=live if dead else None, want_x=False, row_order=torch.from_numpy(order_a).to(DEV))
    c.verify(gwa, None, live, "layout a")
    # layout b: every per-row array permuted
    cb = Lin(n, dim, out_dim, mode, "relu", pad=4, shift=shift, seed=3)
    pt = torch.from_numpy(perm)
    for name in ("agg_h", "out_h", "g_h"):
        h = getattr(c, name).clone()
        v = _view(h, n, h.shape[1] - shift, shift)
        v.copy_(v[pt].clone())
        setattr(cb, name, h)
    if c.sidx is not None:
        cb.sidx = c.sidx[pt]
    elif mode == "concat":
        h = c.self_h.clone()
        v = _view(h, n, h.shape[1] - shift, shift)
        v.copy_(v[pt].clone())
        cb.self_h = h
    db = cb.device_inputs(live)
    rc, order_b = _row_order(nodes_b, live if dead else None, first)
    native.check(rc, "row_order")
    assert np.array_equal(perm[order_b[:live]], order_a[:live])
    gwb, _ = cb.call(db, n_dev=live if dead else None, want_x=False, row_order=torch.from_numpy(order_b).to(DEV))
    assert torch.equal(gwa.view(torch.int32), gwb.view(torch.int32)), "the weight gradient depends on the row layout"


# ================================================================================ 3. mean backward
class Mean:
    """Lists for the mean backward: n rows of up to k ids into a table of T rows.  Empty rows, a hub row, self rows that are
    already in the set / absent / -1; through slot_rows (slots = True) or direct; `wild` ids < 0 and >= T (no slot_rows)."""

    def __init__(self, n, k, T, dim, seed, slots=False, self_rows=True, wild=False, hub=True, ld_pad=4, shift=0):
        rs = np.random.default_rng(seed)
        gen = torch.Generator().manual_seed(seed)
        self.n, self.k, self.T, self.dim, self.slots, self.ld_pad, self.shift = n, k, T, dim, slots, ld_pad, shift
        nbr = rs.integers(0, T, size=(n, k)).astype(np.int64)
        cnt = rs.integers(0, k + 1, size=n)
        cnt[rs.random(n) < 0.3] = k
        cnt[rs.random(n) < 0.1] = 0
        if n > 2:
            cnt[:2] = k
        if hub and n > 1:
            has = np.nonzero(cnt > 0)[0]
            nbr[has, rs.integers(0, k, size=len(has)) % cnt[has]] = T // 2       # the hub: one term from every non-empty row
        if wild:
            m = rs.random((n, k)) < 0.15
            nbr[m] = rs.choice([-1, -7, T, T + 3, 2 ** 30], size=int(m.sum()))
        self.cnt = cnt.astype(np.int32)
        srow = None
        if self_rows:
            srow = rs.integers(0, T, size=n).astype(np.int64)
            dup = np.nonzero((cnt > 0) & (rs.random(n) < 0.3))[0]
            srow[dup] = nbr[dup, rs.integers(0, k, size=len(dup)) % cnt[dup]]   # already in the set (maybe out of range)
            srow[rs.random(n) < 0.15] = -1
            if wild:
                srow[rs.random(n) < 0.1] = T + 1
        self.nbr_row, self.srow = nbr, srow                # effective rows before clamping (what the reference sees)
        self.slot_rows = None
        nbr_dev, srow_dev = nbr, srow
        if slots:
            S = 2 * T + 64
            sperm = rs.permutation(S)
            slot_rows = np.full(S, -1, dtype=np.int32)
            slot_rows[sperm[:T]] = np.arange(T, dtype=np.int32)
            nbr_dev = sperm[nbr]
            if srow is not None:
                srow_dev = np.where(srow < 0, sperm[T + rs.integers(0, T, size=n)], sperm[np.maximum(srow, 0)])
                self.srow = np.where(srow < 0, -1, srow)
            self.slot_rows = torch.from_numpy(slot_rows).to(DEV)
        self.nbr = torch.from_numpy(nbr_dev.astype(np.int32)).to(DEV)
        self.cnt_d = torch.from_numpy(self.cnt).to(DEV)
        self.self_row = None if srow is None else torch.from_numpy(srow_dev.astype(np.int32)).to(DEV)
        self._ref = {}
        self.gbig = torch.randn(n + 1, dim + ld_pad, generator=gen)
        self.g = _view(self.gbig, n, dim, shift)

    def matrix(self, live):
        """Sparse [T, n] fp64: entry (t, r) = the weight row r's gradient adds to table row t (1 / c_r per term)."""
        ts, rs_, ws = [], [], []
        last = self.T - 1
        for r in range(live):
            c = int(self.cnt[r])
            ids = [int(x) for x in self.nbr_row[r, :c]]
            s = -1 if self.srow is None else int(self.srow[r])
            extra = s >= 0 and s not in ids
            ceff = c + int(extra)
            if ceff == 0:
                continue
            for t in ids + ([s] if extra else []):
                ts.append(min(max(t, 0), last)); rs_.append(r); ws.append(1.0 / ceff)
        idx = torch.tensor([ts, rs_], dtype=torch.int64).reshape(2, -1)
        return torch.sparse_coo_tensor(idx, torch.tensor(ws, dtype=torch.float64), (self.T, self.n)).coalesce()

    def reference(self, live):
        if live not in self._ref:
            self._ref[live] = self._reference(live)
        return self._ref[live]

    def _reference(self, live):
        M = self.matrix(live)
        g = self.g.double()
        return torch.sparse.mm(M, g), torch.sparse.mm(M, g.abs()), M

    def run(self, det, n_dev=None, trd=None, out_pad=4):
        L = _lib()
        ld = self.dim + out_pad
        gt = torch.full((self.T, ld), SENTINEL if det else 0.0, device=DEV)
        if not det:
            gt[:, self.dim:] = SENTINEL
        gd = self.gbig.to(DEV)
        gp = ctypes.c_void_p(gd.data_ptr() + 4 * self.shift)
        nd = None if n_dev is None else torch.tensor([n_dev], dtype=torch.int32, device=DEV)
        if det:
            need = L.sage_gather_mean_backward_workspace_bytes(self.n, self.k, self.T)
            assert need > 0
            ws = torch.empty(need, dtype=torch.uint8, device=DEV)
            td = None if trd is None else torch.tensor([trd], dtype=torch.int32, device=DEV)
            native.check(L.sage_gather_mean_backward_ws(gp, gd.shape[1], self.dim, P(self.nbr), P(self.cnt_d), self.k, self.n, P(nd),
                                                        P(self.slot_rows), P(self.self_row), P(gt), self.T, P(td), ld, P(ws), need,
                                                        native.stream_handle()), "gather_mean_backward_ws")
        else:
            native.check(L.sage_gather_mean_backward(gp, gd.shape[1], self.dim, P(self.nbr), P(self.cnt_d), self.k, self.n, P(nd),
                                                     P(self.slot_rows), P(self.self_row), P(gt), self.T, ld, native.stream_handle()),
                         "gather_mean_backward")
        _sync()
        return gt

    def verify(self, gt, live, trows, what):
        want, A, _ = self.reference(live)
        _check(gt[:trows, :self.dim], want[:trows], A[:trows], what)
        _untouched(gt[:, self.dim:], what + " padding columns")
        _untouched(gt[trows:], what + " table rows past table_rows_dev")


# (dim, k, n, T, slots, wild): dims reach det_sum_kernel<8> (< 64), <16> (64..127), <32> (128..255), <64> (>= 256)
MEAN_CASES = [
    (4, 1, 300, 200, False, False), (60, 9, 1000, 700, True, False), (64, 64, 700, 3000, False, False),
    (124, 65, 400, 9000, True, False), (128, 130, 300, 5000, False, False), (252, 9, 4000, 2000, False, False),
    (256, 25, 2000, 20000, True, False), (260, 130, 200, 1000, False, True), (60, 9, 1000, 700, False, True),
]


def mean_checks(cases=MEAN_CASES):
    for dim, k, n, T, slots, wild in cases:
        c = Mean(n, k, T, dim, seed=dim * 31 + k, slots=slots, wild=wild)
        tag = f"dim={dim} k={k} n={n} T={T} slots={slots} wild={wild}"
        for n_dev, trd in ((None, None), (n - 37, T - 11), (0, None), (n + 5, T + 5)):
            live, trows = min(n if n_dev is None else n_dev, n), min(T if trd is None else trd, T)
            a = c.run(True, n_dev, trd)
            c.verify(a, live, trows, tag + f" _ws n_dev={n_dev} rows_dev={trd}")
            assert torch.equal(a.view(torch.int32), c.run(True, n_dev, trd).view(torch.int32)), tag + ": _ws not reproducible"
            c.verify(c.run(False, n_dev), live, T, tag + f" legacy n_dev={n_dev}")


@pytest.mark.parametrize("case", MEAN_CASES, ids=lambda c: "d{}-k{}-n{}-T{}-slots{}-wild{}".format(*c))
def test_mean_backward_both_kernels_match_fp64(case):
    mean_checks([case])


def test_mean_backward_odd_widths_legacy_and_tiny_tables():
    """The legacy kernel at an odd dim and odd ld, shifted 4 bytes; both kernels with one table row (every id clamps to it) and
    with no self rows at all."""
    c = Mean(500, 9, 300, 51, seed=5, ld_pad=3, shift=1)
    c.verify(c.run(False, out_pad=1), 500, 300, "legacy dim 51")
    for det in (True, False):
        c = Mean(300, 9, 1, 64, seed=6, wild=True)
        c.verify(c.run(det), 300, 1, f"table_rows 1 det={det}")
        c = Mean(300, 9, 50, 8, seed=7, self_rows=False)
        c.verify(c.run(det), 300, 50, f"no self rows det={det}")


@pytest.mark.parametrize("wild", [False, True])
@pytest.mark.parametrize("det", [True, False])
def test_mean_backward_is_the_adjoint_of_the_forward(det, wild):
    """<gather_mean(T), G> == <T, gather_mean_backward(G)> in fp64 within the bound, for in-range ids and for ids < 0 / >= the
    table and self rows past the table (which the forward clamps)."""
    from sage355 import ops
    dim, n, k, T = 64, 3000, 9, 800
    c = Mean(n, k, T, dim, seed=11 + int(wild), wild=wild, ld_pad=0)
    tab = torch.randn(T, dim, generator=torch.Generator().manual_seed(2))
    fwd = ops.gather_mean(tab.to(DEV), c.nbr, c.cnt_d, slot_rows=c.slot_rows, self_row=c.self_row).double().cpu()
    bwd = c.run(det, out_pad=0).double().cpu()
    G, Td = c.g.double(), tab.double()
    lhs, rhs = float((fwd * G).sum()), float((Td * bwd).sum())
    _, A, M = c.reference(n)
    bound = BOUND * float((Td.abs() * A).sum())
    assert abs(lhs - rhs) <= bound, f"<F(T), G> = {lhs}, <T, B(G)> = {rhs}: differ by {abs(lhs - rhs):.3g} > {bound:.3g}"
    want = torch.sparse.mm(M, G)
    _check(bwd, want, A, "adjoint case")


# ================================================================================ 4. layer-1 weight gradient of the 2-layer stack
class TwoHop:
    """Inputs of sage_two_hop_grad_w1: batch seeds, n1 layer-1 rows (the seeds' own rows first), row2 / cnt2 into them,
    self_row2 (gcn: the seed's own row, in the set or not; concat: optional).  Rows no live term references hold NaN in h1,
    agg1 and (concat) their table row; for gcn row 0 is one of them (the padded terms of a trip read row 0)."""

    def __init__(self, batch, k2, h1, d0, concat, act, seed, self_rows=True, pad=4, empty=0.1):
        rs = np.random.default_rng(seed)
        gen = torch.Generator().manual_seed(seed)
        self.batch, self.k2, self.h1d, self.d0, self.concat, self.act, self.pad = batch, k2, h1, d0, concat, act, pad
        start = 0 if concat else 1                        # gcn: row 0 is never referenced; the seeds' own rows follow it
        n1 = start + batch + max(8, batch * min(k2, 6))
        self.n1 = n1
        pool = np.arange(start, n1)
        row2 = rs.choice(pool, size=(batch, k2)).astype(np.int64)
        for r in range(batch):                            # distinct ids within a row (the sampler's sets)
            row2[r] = rs.choice(pool, size=k2, replace=False) if len(pool) >= k2 else row2[r]
        cnt2 = rs.integers(0, k2 + 1, size=batch)
        cnt2[rs.random(batch) < 0.3] = k2
        cnt2[rs.random(batch) < empty] = 0
        cnt2[0] = k2
        srow = None
        if self_rows:
            srow = np.arange(batch, dtype=np.int64) + start
            dup = np.nonzero((cnt2 > 0) & (rs.random(batch) < 0.3))[0]
            srow[dup] = row2[dup, rs.integers(0, k2, size=len(dup)) % cnt2[dup]]
            srow[rs.random(batch) < 0.1] = -1
        self.row2, self.cnt2, self.srow = row2, cnt2.astype(np.int32), srow
        self.nodes = rs.permutation(n1 + 100)[:n1].astype(np.int32)
        self.Ntab = n1 + 100
        self.tab_h = torch.randn(self.Ntab, d0 + pad, generator=gen)
        self.h1_h = _act_inputs(gen, n1, h1 + pad, act)
        self.agg_h = torch.randn(n1, d0 + pad, generator=gen)
        self.mult = 2 if concat else 1
        self.gx_h = torch.randn(batch, self.mult * h1 + pad, generator=gen)
        self.K1 = self.mult * d0
        self.g0 = torch.randn(h1, self.K1, generator=gen)
        # rows no live term references -> NaN
        ref = np.zeros(n1, dtype=bool)
        if concat:
            ref[:batch] = True
        for r in range(batch):
            ref[row2[r, :cnt2[r]]] = True
            if srow is not None and srow[r] >= 0:
                ref[srow[r]] = True
        self.dead = np.nonzero(~ref)[0]
        for t in self.dead:
            self.h1_h[t] = float("nan")
            self.agg_h[t] = float("nan")
            if concat:
                self.tab_h[self.nodes[t]] = float("nan")

    def terms(self):
        """(t, r, column offset, weight) of every live term, fp64 weights."""
        out = []
        off_agg = self.h1d if self.concat else 0
        for r in range(self.batch):
            c = int(self.cnt2[r])
            ids = [int(x) for x in self.row2[r, :c]]
            s = -1 if self.srow is None else int(self.srow[r])
            extra = s >= 0 and s not in ids
            ceff = max(c + int(extra), 1)
            if self.concat:
                out.append((r, r, 0, 1.0))
            for t in ids + ([s] if extra else []):
                out.append((t, r, off_agg, 1.0 / ceff))
        return out

    def reference(self):
        h1 = self.h1_h[:, :self.h1d]
        gx = self.gx_h.double()
        gh = torch.zeros(self.n1, self.h1d, dtype=torch.float64)
        gha = torch.zeros_like(gh)
        terms = self.terms()
        for off in sorted({o for _, _, o, _ in terms}):
            sel = [(t, r, w) for t, r, o, w in terms if o == off]
            idx = torch.tensor([[t for t, _, _ in sel], [r for _, r, _ in sel]], dtype=torch.int64)
            M = torch.sparse_coo_tensor(idx, torch.tensor([w for _, _, w in sel], dtype=torch.float64), (self.n1, self.batch)).coalesce()
            gh += torch.sparse.mm(M, gx[:, off:off + self.h1d])
            gha += torch.sparse.mm(M, gx[:, off:off + self.h1d].abs())
        ap = _act_grad64(torch.nan_to_num(h1, nan=0.0), self.act)
        dz, dza = gh * ap, gha * ap
        x = self.agg_h[:, :self.d0].double()
        if self.concat:
            x = torch.cat([self.tab_h[torch.from_numpy(self.nodes).long(), :self.d0].double(), x], 1)
        x = torch.nan_to_num(x, nan=0.0)                  # dead rows: dz is 0 there
        return dz.t() @ x, dza.t() @ x.abs()

    def run(self, ws_bytes=None, ldgw=None, relabel=None):
        L = _lib()
        row2, srow, nodes, h1h, aggh = self.row2, self.srow, self.nodes, self.h1_h, self.agg_h
        if relabel is not None:                           # new row of old row t: relabel[t]
            inv = np.argsort(relabel)
            row2 = relabel[row2]
            srow = None if srow is None else np.where(srow >= 0, relabel[np.maximum(srow, 0)], -1)
            nodes = nodes[inv]
            h1h, aggh = h1h[torch.from_numpy(inv)], aggh[torch.from_numpy(inv)]
        ldgw = ldgw or self.K1 + 3
        gw = torch.full((self.h1d, ldgw), SENTINEL)
        gw[:, :self.K1] = self.g0
        gw = gw.to(DEV)
        d = {k: v.to(DEV) for k, v in dict(gx=self.gx_h, h1=h1h, agg=aggh, tab=self.tab_h).items()}
        r2 = torch.from_numpy(row2.astype(np.int32)).to(DEV)
        c2 = torch.from_numpy(self.cnt2).to(DEV)
        s2 = None if srow is None else torch.from_numpy(srow.astype(np.int32)).to(DEV)
        nd = torch.from_numpy(nodes).to(DEV)
        need = L.sage_two_hop_grad_w1_workspace_bytes(self.batch, self.k2, self.d0, int(self.concat), self.h1d)
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        rc = L.sage_two_hop_grad_w1(P(d["gx"]), d["gx"].shape[1], P(r2), P(c2), self.k2, P(s2), self.batch, P(d["h1"]), d["h1"].shape[1],
                                    self.h1d, ACT[self.act], P(d["agg"]), d["agg"].shape[1], self.d0, int(self.concat), P(d["tab"]),
                                    d["tab"].shape[1], P(nd), P(gw), ldgw, P(ws), need if ws_bytes is None else ws_bytes,
                                    native.stream_handle())
        _sync()
        return rc, gw

    def verify(self, gw, what):
        want, A = self.reference()
        _check(gw[:, :self.K1], want, A, what, g0=self.g0)
        _untouched(gw[:, self.K1:], what + " padding columns")


# (batch, k2, h1, d0, concat, act, self_rows)
TWO_HOP_CASES = [
    (1, 1, 4, 4, False, "relu", True), (3, 9, 52, 60, True, "sigmoid", False), (5, 25, 128, 252, False, "none", True),
    (300, 26, 132, 256, True, "relu", True), (300, 64, 256, 260, False, "sigmoid", True), (300, 9, 128, 1436, False, "relu", True),
    (64, 9, 52, 1436, True, "none", False), (2000, 64, 52, 60, False, "relu", True), (5000, 25, 128, 4, True, "relu", False),
    (5, 1, 256, 256, True, "sigmoid", True), (300, 25, 4, 60, True, "none", True),
]


def two_hop_checks(cases=TWO_HOP_CASES):
    for batch, k2, h1, d0, concat, act, self_rows in cases:
        c = TwoHop(batch, k2, h1, d0, concat, act, seed=batch * 7 + k2, self_rows=self_rows)
        tag = f"batch={batch} k2={k2} h1={h1} d0={d0} concat={concat} {act} self_rows={self_rows}"
        rc, gw = c.run()
        native.check(rc, "two_hop_grad_w1")
        c.verify(gw, tag)
        rc, gw2 = c.run()
        assert torch.equal(gw.view(torch.int32), gw2.view(torch.int32)), tag + ": not reproducible"
        first = batch if concat else 0
        rel = np.arange(c.n1)
        rel[first:] = first + np.random.default_rng(batch).permutation(c.n1 - first)
        rc, gw3 = c.run(relabel=rel)
        assert torch.equal(gw.view(torch.int32), gw3.view(torch.int32)), tag + ": depends on the frontier's row labels"


@pytest.mark.parametrize("case", TWO_HOP_CASES, ids=lambda c: "b{}-k{}-h{}-d{}-cat{}-{}-self{}".format(*c))
def test_two_hop_grad_w1_matches_fp64(case):
    two_hop_checks([case])


# ================================================================================ 5. launch tunables
CHILD = r"""
import sys
sys.path[:0] = [{repo!r}, {repo!r} + "/graphsage-simple_amd", {repo!r} + "/tests"]
import test_gpu_backward_kernels as t
{body}
print("BWD_CHILD_OK")
"""
DIRECT_BODY = ("t.linear_checks([c for c in t.LIN_CASES if c[6] == 0 and c[1] % 2 == 0 and c[2] % 2 == 0 and c[0] > 60], legacy=False)\n"
               "t.two_hop_checks([c for c in t.TWO_HOP_CASES if c[0] >= 300])")
GENERIC_BODY = "t.linear_checks([c for c in t.LIN_CASES if c[6] == 1 or c[1] % 2 == 1 or c[2] % 2 == 1])"


@pytest.mark.parametrize("env,body", [({"SAGE_BWD_DIRECT_BLOCKS": "16"}, DIRECT_BODY), ({"SAGE_BWD_DIRECT_BLOCKS": "1024"}, DIRECT_BODY),
                                      ({"SAGE_BWD_BLOCKS": "16"}, GENERIC_BODY)],
                         ids=["direct16", "direct1024", "generic16"])
def test_backward_kernels_behind_the_launch_tunables(env, body, tmp_path):
    """Fewer and more row splits for the direct and edge kernels (blocks then loop over several chunks), and few splits for the
    generic and legacy weight gradients.  Read once per process: one child process per setting, one at a time."""
    script = tmp_path / "child.py"
    script.write_text(CHILD.format(repo=REPO, body=body))
    e = dict(os.environ)
    e.update(env)
    res = subprocess.run([sys.executable, str(script)], env=e, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "BWD_CHILD_OK" in res.stdout, res.stdout[-2000:] + res.stderr[-3000:]


# ================================================================================ 6. refusals without a launch
def test_refusals_leave_every_output_alone():
    L = _lib()
    st = native.stream_handle()
    # linear_act_backward_ws: short and misaligned workspace
    c = Lin(300, 64, 52, "gcn", "relu")
    d = c.device_inputs(300)
    need = L.sage_linear_act_backward_workspace_bytes(300, 64, 0, 52)
    wsb = torch.empty(need + 64, dtype=torch.uint8, device=DEV)
    for ptr, size in ((wsb.data_ptr(), need - 4), (wsb.data_ptr() + 4, need)):
        gw = torch.full((52, 64), SENTINEL, device=DEV)
        gx = torch.full((300, 64), SENTINEL, device=DEV)
        rc = L.sage_linear_act_backward_ws(None, 0, None, P(d["agg"]), d["agg"].shape[1], 64, P(d["w"]), d["w"].shape[1], 52, RELU,
                                           P(d["out"]), d["out"].shape[1], P(d["g"]), d["g"].shape[1], 300, None, P(gw), 64, P(gx), 64,
                                           None, ctypes.c_void_p(ptr), size, st)
        _sync()
        assert rc != 0
        _untouched(gw, "grad_weight after a refused call")
        _untouched(gx, "grad_x after a refused call")
    # gather_mean_backward_ws: short workspace, misaligned grad_agg / grad_table, ld % 4 != 0
    m = Mean(200, 9, 100, 64, seed=1)
    need = L.sage_gather_mean_backward_workspace_bytes(200, 9, 100)
    wsb = torch.empty(need, dtype=torch.uint8, device=DEV)
    gd = m.gbig.to(DEV)
    for gptr, ldg, tshift, ld, size in ((gd.data_ptr(), gd.shape[1], 0, 68, need - 256), (gd.data_ptr() + 4, gd.shape[1], 0, 68, need),
                                        (gd.data_ptr(), gd.shape[1], 1, 68, need), (gd.data_ptr(), gd.shape[1], 0, 66, need),
                                        (gd.data_ptr(), 66, 0, 68, need)):
        gt = torch.full((100 * 68 + 8,), SENTINEL, device=DEV)
        rc = L.sage_gather_mean_backward_ws(ctypes.c_void_p(gptr), ldg, 64, P(m.nbr), P(m.cnt_d), 9, 200, None, None, P(m.self_row),
                                            ctypes.c_void_p(gt.data_ptr() + 4 * tshift), 100, None, ld, P(wsb), size, st)
        _sync()
        assert rc != 0
        _untouched(gt, "grad_table after a refused call")
    # two_hop_grad_w1: short workspace, misaligned h1 / agg1, ld not a multiple of 4
    c = TwoHop(64, 9, 52, 60, False, "relu", seed=2)
    rc, gw = c.run(ws_bytes=L.sage_two_hop_grad_w1_workspace_bytes(64, 9, 60, 0, 52) - 4)
    assert rc == native.ENOSPACE
    _check(gw[:, :c.K1], torch.zeros(52, 60, dtype=torch.float64), torch.zeros(52, 60), "grad_w1 after a refused call", g0=c.g0)
    _untouched(gw[:, c.K1:], "grad_w1 padding after a refused call")
    h1d, aggd, gxd = c.h1_h.to(DEV), c.agg_h.to(DEV), c.gx_h.to(DEV)
    r2 = torch.from_numpy(c.row2.astype(np.int32)).to(DEV)
    c2 = torch.from_numpy(c.cnt2).to(DEV)
    s2 = torch.from_numpy(c.srow.astype(np.int32)).to(DEV)
    need = L.sage_two_hop_grad_w1_workspace_bytes(64, 9, 60, 0, 52)
    ws = torch.empty(need + 16, dtype=torch.uint8, device=DEV)
    base = dict(gx=gxd.data_ptr(), ldgx=gxd.shape[1], h1=h1d.data_ptr(), ldh=h1d.shape[1], agg=aggd.data_ptr(), lda=aggd.shape[1],
                ws=ws.data_ptr())
    for change in (dict(h1=h1d.data_ptr() + 4), dict(agg=aggd.data_ptr() + 8), dict(gx=gxd.data_ptr() + 4), dict(ws=ws.data_ptr() + 4),
                   dict(ldh=h1d.shape[1] - 1), dict(lda=aggd.shape[1] - 2), dict(ldgx=gxd.shape[1] - 3)):
        a = dict(base, **change)
        gw = torch.full((52, 64), SENTINEL, device=DEV)
        rc = L.sage_two_hop_grad_w1(ctypes.c_void_p(a["gx"]), a["ldgx"], P(r2), P(c2), 9, P(s2), 64, ctypes.c_void_p(a["h1"]), a["ldh"], 52,
                                    RELU, ctypes.c_void_p(a["agg"]), a["lda"], 60, 0, None, 0, None, P(gw), 64,
                                    ctypes.c_void_p(a["ws"]), need, st)
        _sync()
        assert rc != 0, change
        _untouched(gw, f"grad_w1 after a refused call {change}")
