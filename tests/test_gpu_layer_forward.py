"""sage_layer_forward (csrc/sage_fused.hip), called directly, against the fp64 oracle at the shapes where its kernels go wrong.

The oracle is ref_sparse.gather_mean then ref_sparse.linear_act on the same lists.  An empty row's expected value comes from the
any_nonempty flag passed to the kernel (NaN if it is 1, zeros if it is 0 or NULL), not from the batch.  Tolerance:
|got - want| <= 1e-5 * max|pre-activation row|, NaN patterns equal (the rule of test_linear_act_matches_oracle).

Dispatch (sage_launch_layer_fused, default build): KP = 64 / 128 / 256 for dim <= 64 / <= 128 / <= 256, then by n and concat:

    cell (KP, concat, n)      instantiation                                     MATRIX rows (dim < KP, dim == KP)
    64,  gcn,    n < 8192     layer_tile16_kernel<64, false, 7, WAVES>            (60, 64)
    64,  concat, n < 8192     layer_tile16_kernel<64, true, 7, WAVES>             (4, 64)
    128, gcn,    n < 8192     layer_tile16_kernel<128, false, 7, WAVES>           (100, 128)
    128, concat, n < 8192     layer_tile16_kernel<128, true, 7, WAVES>            (68, 128)
    256, gcn,    n < 8192     layer_fused_kernel<256, 32, 8, true, false>         (200, 256)
    256, concat, n < 8192     layer_fused_kernel<256, 32, 8, true, true>          (132, 256)
    64,  gcn,    n >= 8192    layer_fused_kernel<64, 64, 4, true, false>          (60, 64)
    64,  concat, n >= 8192    layer_fused_kernel<64, 64, 4, true, true>           (4, 64)
    128, gcn,    n >= 8192    layer_fused_kernel<128, 64, 4, true, false>         (100, 128)
    128, concat, n >= 8192    layer_fused_kernel<128, 64, 4, true, true>          (68, 128)
    256, gcn,    n >= 8192    layer_fused_kernel<256, 32, 4, false, false>        (252, 256)
    256, concat, n >= 8192    layer_fused_kernel<256, 32, 4, true, true>          (132, 256)

WAVES is the SAGE_T16_WAVES tunable (8 by default, 16); the tile16 kernel's persistent grid is SAGE_T16_GRID blocks.  Both are read
once per process, so the other settings run in child processes (test_tile16_kernel_behind_the_launch_tunables).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import ref_sparse
from sage355 import native, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-5
SENTINEL = -31.5
ACT = {"relu": ops.ACT_RELU, "sigmoid": ops.ACT_SIGMOID, "none": ops.ACT_NONE}


def _prime_at_least(x):
    x = max(int(x), 3)
    while any(x % p == 0 for p in range(2, int(x ** 0.5) + 1)):
        x += 1
    return x


def _bits(t):
    return t.contiguous().view(torch.int32)


class Case:
    """One layer call's inputs, host copies for the oracle and device tensors for the kernel.

    Table rows [0, P) are the sampled population (P prime: row r's ids perm[(base_r + step_r * j) mod P] are distinct for j < P);
    row P is a hub that one in four rows also points at.  The table is a column slice (ld = dim + 16, starting 16 bytes in) of a
    wider array, W a column slice (ldw = m * dim + 8), out a column slice (ldo = out_dim + 3) prefilled with SENTINEL.
    slots: neighbour ids and self rows are hash slots, resolved through slot_rows (a few self slots are unmapped: no self row).
    self_rows: self_row given directly as table rows (some -1: none).  In both, rows whose own row is already among their
    sampled entries exist and must not count it twice.  empty: fraction of rows with cnt == 0.  positive: table and W drawn
    from [0, 1), so no output is a cancelling sum (a one-column row max is then a fair scale for the fp32 error)."""

    def __init__(self, dim, n, k, out_dim, concat, seed, self_index=True, slots=False, self_rows=False, empty=0.1, positive=False):
        rs = np.random.default_rng(seed)
        gen = torch.Generator().manual_seed(seed)
        self.dim, self.n, self.k, self.out_dim, self.concat = dim, n, k, out_dim, concat
        P = _prime_at_least(max(n + 40, 2 * k + 3, 301))
        T = P + 1
        rand = torch.rand if positive else torch.randn
        big = rand(T, dim + 16, generator=gen)
        self.table = big.to(DEV)[:, 4:4 + dim]
        self.table64 = big[:, 4:4 + dim].double()
        m = 2 if concat else 1
        wbig = rand(out_dim, m * dim + 8, generator=gen) / np.sqrt(m * dim)
        self.w = wbig.to(DEV)[:, :m * dim]
        self.w64 = wbig[:, :m * dim].double()
        perm = rs.permutation(P)
        base = rs.integers(0, P, size=n)
        step = rs.integers(1, P, size=n)
        nbr = perm[(base[:, None] + step[:, None] * np.arange(k)[None, :]) % P].astype(np.int64)
        cnt = rs.integers(0, k + 1, size=n)
        cnt[rs.random(n) < 0.25] = k                            # full rows
        cnt[rs.random(n) < empty] = 0
        cnt[:min(n, 2)] = k
        hub = np.nonzero((cnt > 0) & (rs.random(n) < 0.25))[0]
        nbr[hub, rs.integers(0, k, size=len(hub)) % cnt[hub]] = P
        self.nbr_row, self.cnt = nbr, cnt.astype(np.int32)
        # concat self panel: self_index a permutation into the (taller) table, or row r itself
        self.self_idx = None
        if concat and self_index:
            self.self_idx = rs.permutation(T)[:n].astype(np.int32)
        self.self_panel = (self.self_idx if self.self_idx is not None else np.arange(n)) if concat else None
        # set-union self row
        self.self_eff = None
        self.slot_rows = self.self_row = None
        nbr_dev = nbr
        if slots or self_rows:
            srow = rs.integers(0, T, size=n)
            dup = np.nonzero((cnt > 0) & (rs.random(n) < 0.3))[0]       # self already sampled
            srow[dup] = nbr[dup, rs.integers(0, k, size=len(dup)) % cnt[dup]]
            none = rs.random(n) < 0.1
            self.self_eff = np.where(none, -1, srow)
            if slots:
                S = 2 * T + 64
                sperm = rs.permutation(S)
                slot_rows = np.full(S, -1, dtype=np.int32)
                slot_rows[sperm[:T]] = np.arange(T, dtype=np.int32)
                nbr_dev = sperm[nbr]
                self_slot = np.where(none, sperm[T + rs.integers(0, T, size=n)], sperm[srow])   # unmapped slot: no self row
                self.slot_rows = torch.from_numpy(slot_rows).to(DEV)
                self.self_row = torch.from_numpy(self_slot.astype(np.int32)).to(DEV)
            else:
                self.self_row = torch.from_numpy(self.self_eff.astype(np.int32)).to(DEV)
        self.nbr = torch.from_numpy(nbr_dev.astype(np.int32)).to(DEV)
        self.cnt_d = torch.from_numpy(self.cnt).to(DEV)
        self.self_index = None if self.self_idx is None else torch.from_numpy(self.self_idx).to(DEV)

    def oracle(self, act, flag):
        """-> (want, pre) [n, out_dim] fp64."""
        agg = ref_sparse.gather_mean(self.table64, self.nbr_row, self.cnt)
        has_self = np.zeros(self.n, dtype=bool) if self.self_eff is None else self.self_eff >= 0
        if has_self.any():
            h = np.nonzero(has_self)[0]
            agg[torch.from_numpy(h)] = ref_sparse.gather_mean(self.table64, self.nbr_row[h], self.cnt[h], self_idx=self.self_eff[h])
        empty = torch.from_numpy((self.cnt == 0) & ~has_self)
        agg[empty] = float("nan") if flag == 1 else 0.0
        self_feats = None if not self.concat else self.table64[torch.from_numpy(np.asarray(self.self_panel, dtype=np.int64))]
        pre = ref_sparse.linear_act(self_feats, agg, self.w64, "none")
        return ref_sparse.linear_act(self_feats, agg, self.w64, act), pre

    def run(self, act="relu", flag=1, n_dev=None, w=None, out_dim=None, permute=None):
        out_dim = out_dim or self.out_dim
        obig = torch.full((self.n, out_dim + 3), SENTINEL, device=DEV)
        flag_t = None if flag is None else torch.tensor([flag], dtype=torch.int32, device=DEV)
        ndev_t = None if n_dev is None else torch.tensor([n_dev], dtype=torch.int32, device=DEV)
        nbr, cnt, sidx, srow = self.nbr, self.cnt_d, self.self_index, self.self_row
        if permute is not None:
            p = permute
            nbr, cnt = nbr[p].contiguous(), cnt[p].contiguous()
            sidx = None if sidx is None else sidx[p].contiguous()
            srow = None if srow is None else srow[p].contiguous()
            if self.concat and sidx is None:
                raise ValueError("permuting rows needs an explicit self_index")
        ops.layer_forward(self.table, nbr, cnt, self.w if w is None else w, act=ACT[act], concat=self.concat, self_index=sidx,
                          slot_rows=self.slot_rows, self_row=srow, any_nonempty=flag_t, n_dev=ndev_t, out=obig[:, :out_dim])
        torch.cuda.synchronize()
        return obig

    def check(self, obig, want, pre, rows=None, what=""):
        """Rows [0, rows) against the oracle; rows past it and the ldo padding columns still hold the sentinel."""
        rows = self.n if rows is None else rows
        od = want.shape[1]
        got = obig[:rows, :od].cpu().double()
        w, p = want[:rows], pre[:rows]
        tag = f"{what} dim={self.dim} n={self.n} k={self.k} out_dim={od} concat={self.concat}"
        assert torch.equal(torch.isnan(got), torch.isnan(w)), f"{tag}: NaN pattern differs"
        scale = torch.nan_to_num(p).abs().amax(1, keepdim=True).clamp_min(1e-30)
        err = ((torch.nan_to_num(got) - torch.nan_to_num(w)).abs() / scale).max().item() if rows else 0.0
        assert err <= RTOL, f"{tag}: max |gpu-oracle| / pre-activation rowmax = {err:.3e}"
        assert bool((obig[rows:] == SENTINEL).all()), f"{tag}: a row at or past n_dev = {rows} was written"
        assert bool((obig[:, od:] == SENTINEL).all()), f"{tag}: an ldo padding column was written"
        return err


def _mid_tile_cut(n):
    """A row count that ends inside a tile of 16, 32 and 64 rows (37 = 5 mod 16 and mod 32)."""
    return n // 2 if n < 128 else (n // 2) // 64 * 64 + 37


# (dim, concat, n, k, out_dim, act): two rows per dispatch cell, one with dim < KP and one with dim == KP (table above)
MATRIX = [
    # KP 64 -- tile16 / 64-row fused
    (60, False, 1000, 29, 33, "relu"), (64, False, 777, 28, 128, "sigmoid"),
    (4, True, 1000, 7, 17, "none"), (64, True, 1500, 65, 128, "relu"),
    (60, False, 8193, 29, 31, "relu"), (64, False, 8192 + 63, 15, 128, "relu"),
    (4, True, 8192, 28, 15, "sigmoid"), (64, True, 8193, 65, 127, "relu"),
    # KP 128 -- tile16 / 64-row fused
    (100, False, 999, 14, 127, "relu"), (128, False, 1000, 15, 128, "none"),
    (68, True, 1000, 15, 31, "relu"), (128, True, 1024, 14, 128, "sigmoid"),
    (100, False, 8193, 15, 17, "relu"), (128, False, 8192 + 63, 64, 128, "relu"),
    (68, True, 8192, 29, 33, "relu"), (128, True, 8200, 14, 128, "none"),
    # KP 256 -- 32-row fused (8 waves) / 32-row fused (4 waves)
    (200, False, 1000, 8, 128, "relu"), (256, False, 500, 130, 64, "relu"),
    (132, True, 1000, 7, 100, "sigmoid"), (256, True, 777, 65, 128, "relu"),
    (252, False, 8192 + 31, 7, 128, "relu"), (256, False, 8192 + 33, 8, 33, "none"),
    (132, True, 8192 + 33, 15, 128, "relu"), (256, True, 8192 + 31, 9, 127, "relu"),
]


@pytest.mark.parametrize("dim,concat,n,k,out_dim,act", MATRIX)
def test_every_dispatch_cell_matches_oracle(dim, concat, n, k, out_dim, act):
    """Each cell: the whole batch, then the same call cut at n_dev inside a tile, then the same bits twice, then the rows
    permuted (same n, so the same kernel): the output rows permute bit for bit.  Concat cells read the self panel through a
    self_index permutation at dim == KP and from row r (self_index = None) at dim < KP."""
    c = Case(dim, n, k, out_dim, concat, seed=dim * 7 + n + k, self_index=dim in (64, 128, 256))
    want, pre = c.oracle(act, 1)
    full = c.run(act)
    c.check(full, want, pre, what="full")
    cut = _mid_tile_cut(n)
    c.check(c.run(act, n_dev=cut), want, pre, rows=cut, what=f"n_dev={cut}")
    assert torch.equal(_bits(c.run(act)), _bits(full)), "two identical calls differ"
    if not concat or c.self_index is not None:
        p = torch.randperm(n, generator=torch.Generator().manual_seed(n)).to(DEV)
        assert torch.equal(_bits(c.run(act, permute=p)), _bits(full[p])), "permuting the rows does not permute the output"


# ------------------------------------------------------------------------------ tile16: partial tiles and the launch tunables
def tile16_checks():
    """The tile16 cells (KP 64 / 128, gcn and concat) at 1, 15, 16, 17 and 3000 rows (188 tiles: more than a grid of 64
    blocks, so persistent blocks reuse the LDS tile), each whole and cut at n_dev, with empty rows and the self-row union.
    Run in process and, under other tunables, in child processes."""
    for dim in (60, 64, 100, 128):
        for concat in (False, True):
            for i, n in enumerate((1, 15, 16, 17, 3000)):
                k = (7, 29, 15, 65, 14)[(i + dim) % 5]
                c = Case(dim, n, k, 40 + dim % 7, concat, seed=n * 13 + dim, self_index=i % 2 == 0, self_rows=i % 2 == 1)
                want, pre = c.oracle("relu", 1)
                c.check(c.run("relu"), want, pre, what="tile16")
                if n > 1:
                    cut = _mid_tile_cut(n)
                    c.check(c.run("relu", n_dev=cut), want, pre, rows=cut, what=f"tile16 n_dev={cut}")
                c.check(c.run("relu", n_dev=n + 5), want, pre, what="tile16 n_dev > n")


def test_tile16_partial_tiles_and_n_dev():
    tile16_checks()


TILE16_CHILD = r"""
import sys
sys.path[:0] = [{repo!r}, {repo!r} + "/graphsage-simple_amd", {repo!r} + "/tests"]
import test_gpu_layer_forward as t
t.tile16_checks()
print("TILE16_OK")
"""


@pytest.mark.parametrize("env", [{"SAGE_T16_WAVES": "16"}, {"SAGE_T16_WAVES": "8", "SAGE_T16_GRID": "64"}],
                         ids=lambda e: ",".join(f"{k[5:]}={v}" for k, v in e.items()))
def test_tile16_kernel_behind_the_launch_tunables(env, tmp_path):
    """16-wave blocks (one row per wave), and 8-wave blocks on a 64-block grid (a block's later tiles reuse its LDS tile).
    The tunables are read once per process: one child process per setting, one at a time."""
    script = tmp_path / "tile16.py"
    script.write_text(TILE16_CHILD.format(repo=REPO))
    e = dict(os.environ)
    e.update(env)
    res = subprocess.run([sys.executable, str(script)], env=e, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "TILE16_OK" in res.stdout, res.stdout[-2000:] + res.stderr[-3000:]


# ------------------------------------------------------------------------------ output widths, fanouts, self rows, empty rows
@pytest.mark.parametrize("dim,concat,n", [(64, False, 300), (128, True, 300), (256, False, 300), (200, True, 300),
                                          (68, False, 8193), (256, True, 8192 + 33)])
def test_output_widths(dim, concat, n):
    """out_dim around the 16-column (tile16) and 32-column (fused) output tiles, with ldo > out_dim: the padding columns of
    out keep the sentinel.  Non-negative data: with one or a few output columns the row maximum must not be a cancelling sum."""
    c = Case(dim, n, 9, 128, concat, seed=dim + n, positive=True)
    gen = torch.Generator().manual_seed(dim)
    for od in (1, 15, 17, 31, 33, 127, 128):
        m = 2 if concat else 1
        wbig = torch.rand(od, m * dim + 4, generator=gen) / np.sqrt(m * dim)
        c.w64 = wbig[:, :m * dim].double()
        want, pre = c.oracle("relu", 1)
        c.check(c.run("relu", w=wbig.to(DEV)[:, :m * dim], out_dim=od), want, pre, what="out width")


@pytest.mark.parametrize("k", [1, 7, 8, 14, 15, 16, 17, 28, 29, 32, 33, 64, 65, 130])
def test_fanouts_cross_every_trip_and_page(k):
    """Neighbour lists around one trip of the tile16 gather (NPI x 7 in flight: 28 ids at KP 64, 14 at KP 128), of the 32-row
    kernel (8 in flight at KP 256), of the 64-row kernels' lane-group pages (16 / 32 ids) and of the 64-id pages
    (65, 130: a second and a third page).  cnt is drawn from [0, k] with full rows."""
    for dim, concat in ((60, k % 2 == 1), (128, k % 2 == 0), (256, k % 2 == 1)):
        c = Case(dim, 200, k, 48, concat, seed=k * 3 + dim, self_rows=k % 3 == 0)
        want, pre = c.oracle("relu", 1)
        c.check(c.run("relu"), want, pre, what="fanout")
    if k in (16, 17, 32, 33, 65, 130):
        for dim in (64, 128):
            c = Case(dim, 8193, k, 32, False, seed=k + dim)
            want, pre = c.oracle("relu", 1)
            c.check(c.run("relu"), want, pre, what="fanout, 64-row kernel")


CELLS = [(dim, n) for n in (700, 8192 + 33) for dim in (60, 128, 200)]


@pytest.mark.parametrize("concat", [False, True])
@pytest.mark.parametrize("dim,n", CELLS)
def test_self_row_union_and_slot_rows(dim, n, concat):
    """Hash slots resolved through slot_rows, plus a self row per node (some unmapped: none) that joins the mean unless it is
    already among the sampled entries (aggregators.py:50-51: a set union, not counted twice); then self rows as plain rows."""
    c = Case(dim, n, 11, 64, concat, seed=dim + n + concat, slots=True)
    want, pre = c.oracle("relu", 1)
    c.check(c.run("relu"), want, pre, what="slot_rows + self_row")
    d = Case(dim, n, 11, 64, concat, seed=dim + n + 2, self_rows=True)
    want, pre = d.oracle("relu", 1)
    d.check(d.run("relu", n_dev=_mid_tile_cut(n)), want, pre, rows=_mid_tile_cut(n), what="self_row")


@pytest.mark.parametrize("dim,n", [(60, 500), (128, 500), (256, 500), (64, 8193), (256, 8192 + 31)])
def test_empty_rows_follow_the_flag(dim, n):
    """cnt == 0 without a self row: NaN if *any_nonempty != 0, zeros if it is 0 or NULL -- whatever the batch holds (a mixed
    batch under 0, an all-empty batch under 1).  NaN passes relu and sigmoid as in torch."""
    for concat in (False, True):
        c = Case(dim, n, 10, 40, concat, seed=dim + n + 5, empty=0.3)
        for flag in (1, 0, None):
            for act in ("relu", "sigmoid", "none"):
                want, pre = c.oracle(act, flag)
                c.check(c.run(act, flag=flag), want, pre, what=f"flag={flag} act={act}")
        e = Case(dim, n, 10, 40, concat, seed=dim + n + 6, empty=1.1)
        e.cnt[:] = 0
        e.cnt_d.zero_()
        for flag in (1, 0):
            want, pre = e.oracle("relu", flag)
            out = e.run("relu", flag=flag)
            e.check(out, want, pre, what=f"all-empty flag={flag}")
            assert bool(torch.isnan(out[:, :40]).all()) == (flag == 1)


def test_neighbour_ids_are_clamped_into_the_table():
    """Ids outside [0, table_rows) read the nearest table row (include/sage355.h); only the first cnt entries are read."""
    for dim, n in ((64, 100), (128, 100), (256, 100), (64, 8193)):
        c = Case(dim, n, 9, 32, False, seed=dim + 11)
        T = c.table.shape[0]
        rs = np.random.default_rng(dim)
        wild = c.nbr_row.copy()
        wild[rs.random(wild.shape) < 0.2] = T + 5
        wild[rs.random(wild.shape) < 0.2] = -3
        c.nbr = torch.from_numpy(wild.astype(np.int32)).to(DEV)
        c.nbr_row = np.clip(wild, 0, T - 1)
        want, pre = c.oracle("relu", 1)
        c.check(c.run("relu"), want, pre, what="clamped ids")


# ------------------------------------------------------------------------------ refusals
def test_unsupported_shapes_and_misaligned_views_refuse_without_a_launch():
    """dim % 4 != 0, dim > 256, out_dim > 128: layer_forward_supported says no and layer_forward raises.  A table or weight
    view 4 bytes off 16-byte alignment is refused too (the shape alone is supported: the pointer decides).  out keeps the sentinel."""
    T, n, k = 50, 20, 4
    nbr = torch.randint(0, T, (n, k), dtype=torch.int32, device=DEV)
    cnt = torch.full((n,), k, dtype=torch.int32, device=DEV)
    for dim, out_dim in ((6, 32), (260, 32), (64, 129)):
        assert not ops.layer_forward_supported(dim, out_dim, False) and not ops.layer_forward_supported(dim, out_dim, True)
        for concat in (False, True):
            m = 2 if concat else 1
            out = torch.full((n, out_dim), SENTINEL, device=DEV)
            with pytest.raises(native.SageError):
                ops.layer_forward(torch.randn(T, dim, device=DEV), nbr, cnt, torch.randn(out_dim, m * dim, device=DEV),
                                  concat=concat, out=out)
            torch.cuda.synchronize()
            assert bool((out == SENTINEL).all())
    assert ops.layer_forward_supported(64, 32, False) and ops.layer_forward_supported(64, 32, True)
    big = torch.randn(T, 72, device=DEV)
    wbig = torch.randn(32, 136, device=DEV)
    for concat in (False, True):
        m = 2 if concat else 1
        for table, w in ((big[:, 1:65], wbig[:, :m * 64]), (big[:, :64], wbig[:, 1:1 + m * 64])):
            out = torch.full((n, 32), SENTINEL, device=DEV)
            with pytest.raises(native.SageError):
                ops.layer_forward(table, nbr, cnt, w, concat=concat, out=out)
            torch.cuda.synchronize()
            assert bool((out == SENTINEL).all())
