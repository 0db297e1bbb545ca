"""The generic contraction linear_act_kernel (csrc/sage_linear.hip), act([self | agg] . W^T), element by element against fp64 at its
edge shapes, and the arguments the engine's generic two-launch layers hand it.

A. ops.linear_act alone on util.LINEAR_RUNS: every row count, width and output width that the kernel's masks distinguish (64-row
   tiles of two 32-row accumulators, four waves of 32 columns, 128-column blocks in grid.y, 32-wide K panels, the concat seam
   inside a panel), each in three modes (no self_tab; self_tab row r; self_tab row self_index[r] of a taller table), without a
   device-side row count and with n_dev = n - 3 (rows past it NaN), into a sentinel-filled out.  Every operand is a view one float
   into a wider allocation with an odd pad.  Pre-activation against fp64 in units of 2^-23 sum_k |x_k||w_k|; relu bit-equal to the
   relu of the pre-activation; sigmoid within 2e-7 of fp64 sigmoid of the device's own pre-activation; nothing outside rows
   [0, n_dev) x columns [0, out_dim) of out written.  And NaN / +Inf / -Inf in single entries: classes as torch's fp32 mm, every
   finite output of the same tiles within the bar.
B. (tests/test_linear_act_host.py: the emulation the bar comes from, faithful and broken, on the same data.)
C. TwoHopEngine with generic layers (fused=False: both; fused=True with h2 = 130: layer 2, grid.y = 2) on util.split_graph: h1 and
   out bit-equal to ops.gather_mean + ops.linear_act on the recorded lists, and the finish duty that the kernel carries there.

Bar of the pre-activation (util.linear_bar): twice the worst figure that a plain fp32 accumulation in the kernel's own order -- the
numpy emulation, in both rounding variants; not the kernel -- leaves on the same data, and per case below one eighth of the smallest
single term's share of an output, so that no dropped or misplaced term can pass.  Measured on MI355X: DESIGN.md section 6.
"""
import numpy as np
import pytest
import torch

from sage355 import ops
from sage355.engine import TwoHopEngine
from util import (LINEAR_RUNS, contraction_units, gather_form, linear_bar, linear_case, linear_n_devs, linear_operands,
                  linear_poisoned, split_graph, split_lists)

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -31.5
SIGMOID_BAR = 2e-7                                     # test_sigmoid_activation_matches_torch_over_the_fp32_range's


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------- A. ops.linear_act alone
class Uploaded:
    """One case on the device: the flat allocations and the operand views into them."""

    def __init__(self, c):
        self.c = c
        n, dim, h = c["n"], c["dim"], c["out_dim"]
        k = dim * (1 if c["mode"] == "gcn" else 2)

        def view(name, rows, cols):
            off, ld = c[name]
            return torch.from_numpy(c[name + "_flat"]).to(DEV).as_strided((rows, cols), (ld, 1), off)

        self.agg, self.w = view("agg", n, dim), view("w", h, k)
        self.self_tab = None if c["self"] is None else view("self", c["tab_rows"], dim)
        self.self_index = None if c["self_index"] is None else _i32(c["self_index"])

    def run(self, act, nn):
        """-> (the whole out allocation as numpy, mask of the elements the call may write)"""
        c = self.c
        n, h = c["n"], c["out_dim"]
        off, ldo = c["out"]
        flat = torch.full((c["out_size"],), SENTINEL, device=DEV)
        n_dev = None if nn is None else torch.tensor([nn], dtype=torch.int32, device=DEV)
        ops.linear_act(self.agg, self.w, act=act, self_tab=self.self_tab, self_index=self.self_index, n_dev=n_dev,
                       out=flat.as_strided((n, h), (ldo, 1), off))
        torch.cuda.synchronize()
        may = np.zeros(c["out_size"], dtype=bool)
        live = n if nn is None else nn
        may[(off + ldo * np.arange(live)[:, None] + np.arange(h)[None, :]).ravel()] = True
        return flat.cpu().numpy(), may


def _written(flat, c, live):
    off, ldo = c["out"]
    return flat[off + ldo * np.arange(live)[:, None] + np.arange(c["out_dim"])[None, :]]


def check_case(c, nn, tag):
    """One call's arguments through the three activations -> the pre-activation's worst figure (and asserts)."""
    up = Uploaded(c)
    live = c["n"] if nn is None else nn
    sent = np.float32(SENTINEL).view(np.int32)
    outs = {}
    for act in (ops.ACT_NONE, ops.ACT_RELU, ops.ACT_SIGMOID):
        flat, may = up.run(act, nn)
        assert np.all(flat.view(np.int32)[~may] == sent), \
            f"{tag} act={act}: written outside rows [0, {live}) x columns [0, {c['out_dim']}) of out, at flat offsets {np.nonzero((flat.view(np.int32) != sent) & ~may)[0][:8].tolist()}"
        outs[act] = _written(flat, c, live)
    pre = outs[ops.ACT_NONE]
    bar, figs, share = linear_bar(c, nn=nn)
    worst, where = 0.0, (0, 0)
    if live:
        x, w = linear_operands(c)
        assert not np.isnan(pre).any(), f"{tag}: NaN in rows {np.nonzero(np.isnan(pre).any(1))[0][:8].tolist()}: a row at or past n_dev was read"
        units, _ = contraction_units(pre, x[:live], w)
        worst, where = float(units.max()), np.unravel_index(np.argmax(units), units.shape)
    print(f"LINACT {tag} K={c['dim'] * (1 if c['mode'] == 'gcn' else 2)}: kernel {worst:.2f} x 2^-23 sum|x||w| at row {where[0]} column {where[1]} "
          f"(bar {bar:.2f} = 2 x emulation: fma {figs['fma']:.2f}, mul_add {figs['mul_add']:.2f}; smallest term {share:.0f})")
    assert bar < share / 8, f"{tag}: bar {bar:.2f} is not below an eighth of the smallest term's share {share:.0f}"
    assert worst <= bar, f"{tag}: out[{where[0]}, {where[1]}] is {worst:.2f} x 2^-23 sum|x||w| from fp64, bar {bar:.2f}"
    want_relu = np.where(pre < 0, np.float32(0), pre)
    assert np.array_equal(outs[ops.ACT_RELU].view(np.int32), want_relu.view(np.int32)), f"{tag}: relu is not the relu of the pre-activation"
    if live:
        with np.errstate(over="ignore"):
            want_sig = 1.0 / (1.0 + np.exp(-pre.astype(np.float64)))
        err = float(np.abs(outs[ops.ACT_SIGMOID].astype(np.float64) - want_sig).max())
        assert err <= SIGMOID_BAR, f"{tag}: sigmoid {err:.2e} from fp64 sigmoid of the pre-activation"
    return worst


def _run_id(run):
    n, dim, h, mode, small = run
    return f"n{n}-d{dim}-h{h}-{mode}"


# the check of the list itself (every value in every mode, every out_dim beside a partial accumulator, a seam inside a panel,
# grid.y > 1, a wholly empty tile) needs no GPU: it is defined beside the emulation and collected here as well
from test_linear_act_host import test_cases_reach_every_mask_with_every_value  # noqa: E402,F401


@pytest.mark.parametrize("run", LINEAR_RUNS, ids=_run_id)
def test_linear_act_alone(run):
    n, dim, h, mode, small = run
    c = linear_case(n, dim, h, mode)
    for nn in linear_n_devs(n, small):
        check_case(c if nn is None else linear_poisoned(c, nn), nn, f"n={n} dim={dim} out_dim={h} {mode} n_dev={nn}")


def test_gcn_mode_is_the_agg_half_of_the_concat_weight():
    """Without self_tab the kernel reads W[:, dim:] of the concat W and nothing of a self table: the gcn result on that view is
    bit-equal to the gcn result on a contiguous copy of the half, whatever the other half holds."""
    n, dim, h = 65, 50, 33
    c = linear_case(n, dim, h, "gcn")
    up = Uploaded(c)
    got = ops.linear_act(up.agg, up.w, act=ops.ACT_NONE)
    half = up.w.clone()
    assert half.is_contiguous() and up.w.stride(0) == 2 * dim + 5 and up.w.storage_offset() == 1 + dim
    want = ops.linear_act(up.agg.clone(), half, act=ops.ACT_NONE)
    c2 = dict(c)
    c2["w_flat"] = c["w_flat"].copy()
    off, ldw = c["w"]
    for r in range(h):
        c2["w_flat"][off + r * ldw - dim: off + r * ldw] = np.nan          # the self half, which the gcn mode must not read
    again = ops.linear_act(up.agg, Uploaded(c2).w, act=ops.ACT_NONE)
    torch.cuda.synchronize()
    assert torch.equal(_bits(got), _bits(want)) and torch.equal(_bits(got), _bits(again))


def test_non_finite_entries_stay_in_their_rows_and_columns():
    """n = 65, dim = 50, out_dim = 33, concat through self_index: NaN, +Inf and -Inf in single entries of distinct rows of agg and
    of self_tab, one +Inf in W.  The class of every output is that of torch's fp32 x . W^T on the CPU; every finite output, in the
    same tiles as the others, meets the bar."""
    n, dim, h = 65, 50, 33
    c = linear_case(n, dim, h, "concat_index")
    bar, figs, share = linear_bar(c)
    c = dict(c)
    c["agg_flat"], c["self_flat"], c["w_flat"] = c["agg_flat"].copy(), c["self_flat"].copy(), c["w_flat"].copy()

    def poke(name, row, col, v):
        off, ld = c[name]
        c[name + "_flat"][off + row * ld + col] = v

    idx = c["self_index"]
    for row, col, v in ((3, 0, np.nan), (20, dim - 1, np.inf), (40, 17, -np.inf), (64, 31, np.inf)):
        poke("agg", row, col, v)
    for row, col, v in ((10, dim - 1, np.nan), (33, 0, np.inf), (63, 32, -np.inf)):
        poke("self", int(idx[row]), col, v)
    poke("w", 5, dim + 10, np.inf)
    x, w = linear_operands(c)
    bad_rows = np.nonzero(~np.isfinite(x).all(1))[0]
    assert bad_rows.tolist() == [3, 10, 20, 33, 40, 63, 64] and np.nonzero(~np.isfinite(w).all(1))[0].tolist() == [5]
    up = Uploaded(c)
    flat, may = up.run(ops.ACT_NONE, None)
    assert np.all(flat.view(np.int32)[~may] == np.float32(SENTINEL).view(np.int32))
    got = _written(flat, c, n)
    want = (torch.from_numpy(x) @ torch.from_numpy(w).t()).numpy()
    for name, cls in (("NaN", np.isnan), ("+Inf", np.isposinf), ("-Inf", np.isneginf)):
        assert np.array_equal(cls(got), cls(want)), f"{name} at {np.argwhere(cls(got) != cls(want))[:8].tolist()}, torch's fp32 mm has it elsewhere"
    fin = np.isfinite(want)
    expect_fin = np.ones((n, h), dtype=bool)
    expect_fin[bad_rows] = False
    expect_fin[:, 5] = False
    assert np.array_equal(fin, expect_fin)
    xz, wz = x.copy(), w.copy()
    xz[bad_rows] = 1.0
    wz[5] = 1.0
    units, _ = contraction_units(np.where(fin, got, 0.0), xz, wz)
    worst = float(units[fin].max())
    print(f"LINACT non-finite n={n} dim={dim} out_dim={h} concat_index K={2 * dim}: finite outputs {worst:.2f} x 2^-23 sum|x||w| (bar {bar:.2f})")
    assert bar < share / 8 and worst <= bar, f"a finite output is {worst:.2f} units from fp64, bar {bar:.2f}"


# -------------------------------------------------------------------------------- C. the engine's generic two-launch layers
D0, H1, K1, K2, ROWS = 100, 50, 9, 64, 130
ENGINE_FORMS = [(False, False, 33), (True, False, 33), (False, True, 130), (True, True, 130)]        # (concat, fused, h2)


def _form_id(f):
    return f"{'concat' if f[0] else 'gcn'}-{'fused' if f[1] else 'generic'}-h2_{f[2]}"


class EngineCase:
    """A graph whose degrees are at most the fanouts (util.split_graph: the sets are the neighbourhoods), ROWS layer-1 rows, and
    engines over it whose layer 2 (fused=False: and layer 1) takes the generic gather_mean + linear_act form."""

    def __init__(self, concat, fused, h2):
        self.concat, self.fused, self.h2 = concat, fused, h2
        g = self.g = split_graph(ROWS, K1, concat, False, seed=D0 + ROWS)
        self.b = g["b"]
        self.max_batch = self.b + 3
        m = 2 if concat else 1
        gen = torch.Generator().manual_seed(17 + h2 + m)
        self.table = torch.randn(g["num_nodes"], D0, generator=gen).to(DEV)
        self.w1 = (torch.randn(H1, m * D0, generator=gen) / 10).to(DEV)
        self.w2 = (torch.randn(h2, m * H1, generator=gen) / 7).to(DEV)
        pad = np.zeros(1, dtype=np.int32)
        self.csr = (torch.from_numpy(g["rowptr_in"]).to(DEV), _i32(np.concatenate([g["col_in"], pad])),
                    torch.from_numpy(g["rowptr_out"]).to(DEV), _i32(np.concatenate([g["col_out"], pad])))
        self.seeds = torch.arange(self.max_batch, dtype=torch.int32, device=DEV)

    def engine(self):
        rp_in, col_in, rp_out, col_out = self.csr
        eng = TwoHopEngine(rp_in, col_in, self.table, self.w1, self.w2, K1, K2, concat=self.concat, act1=ops.ACT_RELU, act2=ops.ACT_NONE,
                           nan_empty=True, fused=self.fused, max_batch=self.max_batch, rowptr_outer=rp_out, col_outer=col_out)
        # the forms: layer 2 generic; layer 1 generic without `fused`, the one-launch layer with it; never split
        assert eng.table is self.table and not eng.layout.layer1_split and (eng.d0p, eng.h1p) == (D0, 52)
        assert not (self.fused and ops.layer_forward_supported(eng.h1p, self.h2, self.concat))
        assert ops.layer_forward_supported(eng.d0p, eng.h1p, self.concat)
        return eng


@pytest.fixture(scope="module", params=ENGINE_FORMS, ids=_form_id)
def engine_case(request):
    return EngineCase(*request.param)


def _counters(eng):
    torch.cuda.synchronize()
    return eng._ws_views()("counters").cpu().numpy()


def test_engine_generic_layers_are_the_public_operators_on_the_recorded_lists(engine_case):
    """h1 and out of a forward, bit for bit, from ops.gather_mean then ops.linear_act with the engine's n, n_dev, self_row and
    any_nonempty on what the forward left in the workspace: judges n_off / first_row, self_index = s1_nodes, ldw, ldo and the
    padded widths (h1 = 50 lives in 52 columns).  The kernels themselves are judged in part A and tests/test_gpu_split_layer1.py."""
    ec = engine_case
    concat, b, g = ec.concat, ec.b, ec.g
    eng = ec.engine()
    out = eng.forward(ec.seeds[:b], seed=5)
    it = eng.intermediates()
    ws, L = eng._ws_views(), eng.layout
    counters = ws("counters").clone()
    first = b if concat else 0
    n1 = it["n_s1"]
    assert n1 == ROWS and int(counters[8]) == g["f"] == n1 - first
    s1 = it["s1_nodes"].cpu().numpy().astype(np.int64)
    assert sorted(s1.tolist()) == sorted(g["order"].tolist()) and (not concat or np.array_equal(s1[:b], np.arange(b)))
    want_nbr, want_cnt = split_lists(g, s1, K1)
    cnt1 = it["cnt1"].cpu().numpy()
    assert np.array_equal(cnt1, want_cnt), "the sampler did not take whole neighbourhoods"
    live = np.arange(K1)[None, :] < cnt1[:, None]
    assert np.array_equal(np.sort(np.where(live, it["nbr1"].cpu().numpy(), -1), 1), np.sort(np.where(live, want_nbr, -1), 1))
    assert (cnt1 == 0).sum() == 1                                  # the isolated node: a NaN row of the means
    w1p, w2p = eng._weights()
    assert tuple(w1p.shape) == (52, (2 if concat else 1) * D0) and tuple(w2p.shape) == (ec.h2, (2 if concat else 1) * 52)
    n_dev = (counters[8:9] + first).to(torch.int32)
    h1_ws = ws("h1")                                               # [max_s1, 52]
    if not ec.fused:
        # layer 1: n = max_s1 rows with the device-side count first_row + frontier size; the concat rows' own features by s1_nodes
        agg1 = torch.full((L.max_s1, D0), SENTINEL, device=DEV)
        assert gather_form(D0, eng.table_ld, agg1.stride(0), L.max_s1, K1, agg1.data_ptr() % 16 == 0) == gather_form(D0, eng.table_ld, D0, L.max_s1, K1)
        ops.gather_mean(eng.table, ws("nbr1"), ws("cnt1"), any_nonempty=counters[10:11].clone(), n_dev=n_dev, out=agg1)
        h1 = torch.full((L.max_s1, 52), SENTINEL, device=DEV)
        ops.linear_act(agg1, w1p, act=ops.ACT_RELU, self_tab=eng.table if concat else None, self_index=ws("s1_nodes") if concat else None,
                       n_dev=n_dev, out=h1)
        torch.cuda.synchronize()
        assert torch.isnan(agg1[:n1]).any(1).sum() == 1 and bool((h1[n1:] == SENTINEL).all())
        assert torch.equal(_bits(h1[:n1]), _bits(h1_ws[:n1])), "layer 1 (generic form) is not gather_mean + linear_act on its lists"
        assert bool((torch.nan_to_num(h1_ws[:n1, H1:]) == 0).all())            # relu of the zero weight rows (NaN in the isolated node's row)
    # layer 2: n = batch rows, no device-side count; the 0/0 rule is keyed by the frontier count; the concat rows' own h1 by row r
    row2, cnt2 = ws("row2"), ws("cnt2")
    assert gather_form(52, 52, 52, b, K2) == gather_form(52, h1_ws.stride(0), 52, b, K2, h1_ws.data_ptr() % 16 == 0)
    agg2 = ops.gather_mean(h1_ws, row2, cnt2, any_nonempty=counters[8:9].clone())
    want = torch.full((b, ec.h2 + 3), SENTINEL, device=DEV)
    ops.linear_act(agg2, w2p, act=ops.ACT_NONE, self_tab=h1_ws if concat else None, out=want[:, :ec.h2])
    torch.cuda.synchronize()
    assert torch.equal(_bits(agg2), _bits(eng._view(L.agg2, b * 52, torch.float32).view(b, 52))), "layer 2's means"
    assert torch.equal(_bits(out), _bits(want[:, :ec.h2])), "layer 2 (generic form) is not gather_mean + linear_act on its lists"
    assert bool((want[:, ec.h2:] == SENTINEL).all())
    # the same into a strided out of the caller's
    big = torch.full((b, ec.h2 + 5), SENTINEL, device=DEV)
    eng.forward(ec.seeds[:b], seed=5, out=big[:, 1:1 + ec.h2])
    torch.cuda.synchronize()
    assert torch.equal(_bits(big[:, 1:1 + ec.h2]), _bits(out)) and bool((big[:, 0] == SENTINEL).all()) and bool((big[:, 1 + ec.h2:] == SENTINEL).all())


def test_engine_generic_layer2_carries_the_finish_duty(engine_case):
    """linear_act_kernel as the forward's last kernel (sage_finish_t): its last block zeroes the seven live counters and the ticket,
    leaves the read-back copy, and advances the batch-queue cursor by one -- over grid.x x grid.y blocks."""
    ec = engine_case
    b, g = ec.b, ec.g
    first = b if ec.concat else 0
    eng = ec.engine()
    assert (_counters(eng)[:16] == 0).all()
    eng.forward(ec.seeds[:b], seed=5)
    c = _counters(eng)
    assert (c[:8] == 0).all(), f"live counters after a forward: {c[:8].tolist()}"
    assert c[8] + first == ROWS and c[8] == g["f"]
    # a second forward with other seeds on the used engine against a fresh engine's
    other = torch.flip(ec.seeds[:b], [0])[:max(b - 1, 1)].contiguous()
    got = eng.forward(other, seed=11)
    want = ec.engine().forward(other, seed=11)
    torch.cuda.synchronize()
    assert torch.equal(_bits(got), _bits(want)), "a forward on a used workspace differs from a fresh engine's"
    assert (_counters(eng)[:8] == 0).all()
    # queued forwards: the cursor moves by exactly one per forward and each equals the direct call
    ring = torch.stack([ec.seeds[:b], torch.flip(ec.seeds[:b], [0]), torch.roll(ec.seeds[:b], 1)]).contiguous()
    keys = [21, 2 ** 63 + 22, 23]
    direct = ec.engine()
    eng.set_queue(ring, keys)
    out = torch.empty(b, ec.h2, device=DEV)
    for i in range(4):
        before = int(eng._cursor.item())
        eng.forward_queued(out)
        torch.cuda.synchronize()
        assert int(eng._cursor.item()) == before + 1 == i + 1, f"queued forward {i}: cursor {before} -> {int(eng._cursor.item())}"
        assert (_counters(eng)[:8] == 0).all()
        want = direct.forward(ring[i % 3], seed=keys[i % 3])
        assert torch.equal(_bits(out), _bits(want)), f"queued forward {i} differs from the direct call"
