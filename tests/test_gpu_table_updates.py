"""Feature-table and weight updates reach every engine form.

TwoHopEngine does not always read the caller's tensors: with relabel="degree" it works on a degree-renumbered copy of the table,
with a width, leading dimension or base address the 16-B-per-lane kernels cannot take on a zero-padded copy, for the gcn encoder's
split layer 1 on a slice-major copy, and with padded widths on zero-padded weights; the weights also live on as bf16 planes.  Role
pipelines and captured graphs hold raw pointers to these copies.  Each test below builds every form (forward, sibling, captured
engine, role pipeline idle and with a batch in flight, captured pipeline, the drop-in Encoder pair), runs it, updates the caller's
tensors, makes the call INTEGRATION.md names for that update, runs it again on the same seeds and sampler key, and checks:
(a) bit for bit the output of a freshly built engine on the updated tensors, (b) that fresh output against the fp64 oracle on its
own sampled sets, (c) that the output moved, (d) that the private buffers kept their addresses, (e) that pad columns stay zero.
"""
import random

import numpy as np
import pytest
import torch

from sage355.engine import RolePipeline, TwoHopEngine
from sage355.graph import rmat_graph
from test_gpu_forward import build_modules
from util import assert_close_rowmax, full_table, load_golden, oracle_on_engine_sets, sets_from_padded, torch_two_hop

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEY = 77

# name -> shape of the problem and the form of the table handed to the engine
#   form "plain": a contiguous tensor; "ld257": big[:, :256] of a 257-wide `big` (leading dimension not a multiple of 4);
#   "misaligned": a contiguous tensor whose base is one float past a 16-byte boundary
LAYOUTS = {
    "plain_d256": dict(d0=256, h1=128, concat=False, relabel=None, form="plain", b=2048, k=(15, 25)),
    "relabel_d256": dict(d0=256, h1=128, concat=False, relabel="degree", form="plain", b=2048, k=(15, 25)),
    "relabel_concat_d128": dict(d0=128, h1=128, concat=True, relabel="degree", form="plain", b=1024, k=(10, 20)),
    "pad_d66": dict(d0=66, h1=30, concat=False, relabel=None, form="plain", b=512, k=(10, 20)),
    "pad_d1433": dict(d0=1433, h1=50, concat=False, relabel=None, form="plain", b=256, k=(10, 10)),
    "ld257": dict(d0=256, h1=128, concat=False, relabel=None, form="ld257", b=2048, k=(15, 25)),
    "misaligned": dict(d0=256, h1=128, concat=False, relabel=None, form="misaligned", b=2048, k=(15, 25)),
    "relabel_pad_d66": dict(d0=66, h1=30, concat=False, relabel="degree", form="plain", b=512, k=(10, 20)),
}
UPDATES = ["table_inplace", "table_data", "weights_inplace", "weights_data"]

_GRAPH = {}


def _graph():
    if "g" not in _GRAPH:
        _GRAPH["g"] = rmat_graph(14, 300_000, seed=3)
    return _GRAPH["g"]


def _device_table(host, form):
    n, d = host.shape
    if form == "plain":
        return host.to(DEV)
    if form == "ld257":
        big = torch.zeros(n, d + 1, device=DEV)
        big[:, :d] = host.to(DEV)
        return big[:, :d]
    if form == "misaligned":
        flat = torch.zeros(n * d + 1, device=DEV)
        t = flat[1:].view(n, d)
        t.copy_(host.to(DEV))
        return t
    raise ValueError(form)


def _pointers(e):
    """The private buffers a role pipeline or a captured graph holds the address of."""
    w1, w2 = e._weights()
    bufs = {"table": e.table, "table_sliced": e._table_sliced, "w1": w1, "w2": w2, "w1_prepared": e._w1prep}
    return {k: v.data_ptr() for k, v in bufs.items() if v is not None}


def _pads_are_zero(e):
    w1p, w2p = e._weights()
    m = 2 if e.concat else 1
    pads = [e.table[:, e.d0:], w1p[e.h1:]]
    for c in range(m):
        pads += [w1p[:, c * e.d0p + e.d0:(c + 1) * e.d0p], w2p[:, c * e.h1p + e.h1:(c + 1) * e.h1p]]
    return all(not bool(p.any()) for p in pads if p.numel())


def _same(a, b):
    return torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))


def _assert_layout_taken(name, e, table):
    """The path a layout is there for is the one the engine takes."""
    spec = LAYOUTS[name]
    private = spec["relabel"] is not None or spec["form"] != "plain" or spec["d0"] % 4 != 0
    assert (e.table is not table) == private, f"{name}: private table copy expected={private}"
    assert (e.node_order is not None) == (spec["relabel"] is not None)
    if spec["form"] == "ld257":
        assert table.stride(0) == 257 and e.table_ld == 256
    if spec["form"] == "misaligned":
        assert table.data_ptr() % 16 != 0 and e.table.data_ptr() % 16 == 0
    if spec["d0"] % 4 != 0 or spec["h1"] % 4 != 0:
        assert e._padded and e.table.shape[1] == e.d0p > e.d0
    if spec["d0"] % 32 == 0 and not spec["concat"]:
        assert e.layout.layer1_split == 1 and e._table_sliced is not None, f"{name}: split layer 1 over the slice-major copy expected"


def _rows_to_update(e, seeds, rng):
    """Caller ids of rows the last forward read: seeds, frontier nodes that are not seeds, and nodes read only as layer-1 neighbours."""
    it = e.intermediates()
    first = it["first_frontier_row"]
    s1 = it["s1_nodes"].cpu().numpy()[first:]
    nbr1, cnt1 = it["nbr1"].cpu().numpy()[first:], it["cnt1"].cpu().numpy()[first:]
    inner = nbr1[np.arange(nbr1.shape[1])[None, :] < cnt1[:, None]]
    if e.node_order is not None:
        order = e.node_order.cpu().numpy()
        s1, inner = order[s1], order[inner]
    seed_set = set(seeds.tolist())
    frontier_only = np.array(sorted(set(s1.tolist()) - seed_set))
    inner_only = np.array(sorted(set(inner.tolist()) - set(s1.tolist()) - seed_set))
    assert len(frontier_only) and len(inner_only)
    pick = lambda a, n: rng.choice(a, min(n, len(a)), replace=False)          # noqa: E731
    return torch.from_numpy(np.concatenate([pick(seeds, 32), pick(frontier_only, 64), pick(inner_only, 128)]).astype(np.int64))


@pytest.mark.parametrize("update", UPDATES)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_update_reaches_every_engine_form(layout, update):
    spec = LAYOUTS[layout]
    graph = _graph()
    d0, h1, h2, b, (k1, k2) = spec["d0"], spec["h1"], 64, spec["b"], spec["k"]
    m = 2 if spec["concat"] else 1
    gen = torch.Generator().manual_seed(sum(map(ord, layout)))
    table = _device_table(torch.randn(graph.num_nodes, d0, generator=gen), spec["form"])
    w1 = (torch.randn(h1, m * d0, generator=gen) / np.sqrt(m * d0)).to(DEV)
    w2 = (torch.randn(h2, m * h1, generator=gen) / np.sqrt(m * h1)).to(DEV)
    rng = np.random.default_rng(len(layout))
    seeds_np = rng.choice(np.nonzero(graph.degrees() > 0)[0], b, replace=False)
    seeds = torch.from_numpy(seeds_np.astype(np.int32)).to(DEV)
    rowptr, col = graph.to(DEV)
    kw = dict(concat=spec["concat"], relabel=spec["relabel"])

    def engine():
        return TwoHopEngine(rowptr, col, table, w1, w2, k1, k2, max_batch=b, **kw)

    # ---- every form, run once on the tensors as they are
    eng = engine()
    before = eng.forward(seeds, seed=KEY).clone()
    _assert_layout_taken(layout, eng, table)
    rows = _rows_to_update(eng, seeds_np, rng)
    sib = eng.sibling()
    problems = []
    if not (sib.table is eng.table and sib._table_sliced is eng._table_sliced):
        problems.append("sibling: does not share the private table copies")
    sib_out = sib.forward(seeds, seed=KEY).clone()
    cap = engine()
    cap.set_queue(seeds[None].contiguous(), [KEY])
    cap_out = cap.capture()
    cap.replay()
    cap_before = cap_out.clone()
    pipe_idle = RolePipeline(rowptr, col, table, w1, w2, k1, k2, batch=b, depth=2, **kw)
    idle_out = torch.zeros(2, b, h2, device=DEV)
    pipe_idle.submit(seeds, KEY, idle_out[0])
    pipe_idle.synchronize()
    assert pipe_idle.express_count == 1               # the idle pipe's express lane (after an update the submit that re-derives the
                                                      # copies may find its own refresh still running: either lane, the same bits)
    pipe_cap = RolePipeline(rowptr, col, table, w1, w2, k1, k2, batch=b, depth=2, **kw)
    pcap_out = torch.zeros(2, b, h2, device=DEV)
    graph_cap, cap_stream = pipe_cap.capture(seeds[None].contiguous(), [KEY], pcap_out)
    torch.cuda.synchronize()
    with torch.cuda.stream(cap_stream):
        graph_cap.replay()
    torch.cuda.synchronize()
    pcap_before = pcap_out[0].clone()
    for what, out in (("sibling", sib_out), ("captured engine", cap_before), ("idle pipe", idle_out[0]), ("captured pipe", pcap_before)):
        assert _same(out, before), f"{what} differs from forward before any update"
    pipe_busy = RolePipeline(rowptr, col, table, w1, w2, k1, k2, batch=b, depth=2, **kw)
    busy_out = torch.zeros(2, b, h2, device=DEV)
    torch.cuda.synchronize()
    pipe_busy.submit(seeds, KEY, busy_out[0])         # still in flight when the update is made ...
    pipe_busy.join()                                  # ... which is ordered behind it on the current stream
    owners = {"forward": eng, "captured engine": cap, "idle pipe": pipe_idle.engines[0], "busy pipe": pipe_busy.engines[0],
              "captured pipe": pipe_cap.engines[0]}
    ptrs = {k: _pointers(e) for k, e in owners.items()}

    # ---- the update, on the caller's tensors, then the call INTEGRATION.md names for it
    new_rows = (torch.randn(len(rows), d0, generator=gen) * 2).to(DEV)
    d1 = (torch.randn(w1.shape, generator=gen) * float(w1.std()) * 0.5).to(DEV)
    d2 = (torch.randn(w2.shape, generator=gen) * float(w2.std()) * 0.5).to(DEV)
    if update == "table_inplace":
        table[rows.to(DEV)] = new_rows
    elif update == "table_data":
        table.data[rows.to(DEV)] = new_rows
    elif update == "weights_inplace":
        with torch.no_grad():
            w1.add_(d1)
            w2.add_(d2)
    else:
        w1.data.add_(d1)
        w2.data.add_(d2)

    def soft(what, fn):
        try:
            fn()
        except Exception as exc:                     # one form's failure must not hide the others'
            problems.append(f"{what}: {type(exc).__name__}: {exc}")

    if update == "table_data":
        soft("forward refresh_table", eng.refresh_table)                  # reaches the sibling too (shared copies)
        soft("idle pipe refresh_table", pipe_idle.refresh_table)
        soft("busy pipe refresh_table", pipe_busy.refresh_table)
    if update == "weights_data":
        soft("forward invalidate_weights", eng.invalidate_weights)        # reaches the sibling too
        soft("idle pipe refresh_weights", lambda: pipe_idle.refresh_weights())
        soft("busy pipe refresh_weights", lambda: pipe_busy.refresh_weights())
    if update.startswith("table"):                   # a replay looks at no version counter: any write needs the call
        soft("captured engine refresh_table", cap.refresh_table)
        soft("captured pipe refresh_table", pipe_cap.refresh_table)
    else:
        soft("captured engine refresh_weights", cap.refresh_weights)
        soft("captured pipe refresh_weights", lambda: pipe_cap.refresh_weights())

    # ---- every form again, same seeds and key
    after = {}
    soft("busy pipe submit", lambda: pipe_busy.submit(seeds, KEY, busy_out[1]))
    soft("forward", lambda: after.__setitem__("forward", eng.forward(seeds, seed=KEY).clone()))
    soft("sibling", lambda: after.__setitem__("sibling", sib.forward(seeds, seed=KEY).clone()))
    soft("captured engine", lambda: after.__setitem__("captured engine", cap.replay().clone()))
    soft("idle pipe submit", lambda: (pipe_idle.submit(seeds, KEY, idle_out[1]), pipe_idle.synchronize()))
    torch.cuda.synchronize()
    with torch.cuda.stream(cap_stream):
        graph_cap.replay()
    torch.cuda.synchronize()
    pipe_busy.synchronize()
    after.update({"idle pipe": idle_out[1], "busy pipe": busy_out[1], "captured pipe": pcap_out[0]})
    assert _same(busy_out[0], before), "the batch in flight at the update saw the new values"

    # ---- the yardsticks: a fresh engine on the updated tensors, and the fp64 oracle on its own sets
    fresh = engine()
    want = fresh.forward(seeds, seed=KEY).clone()
    assert_close_rowmax(want.cpu(), oracle_on_engine_sets(fresh, table, w1, w2, seeds_np), what=f"{layout} {update}: fresh engine vs fp64")
    assert not _same(want, before), "the update changed nothing: it cannot tell a fresh copy from a stale one"
    for what, out in after.items():
        if not _same(out, want):
            stale = _same(out, before)
            problems.append(f"{what}: output differs from a fresh engine on the updated tensors" + (" (= the stale output)" if stale else ""))
    for what, e in owners.items():
        now = _pointers(e)
        if now != ptrs[what]:
            problems.append(f"{what}: private buffers moved {ptrs[what]} -> {now}")
        if not _pads_are_zero(e):
            problems.append(f"{what}: pad columns of a private copy are not zero")
    assert not problems, f"{layout} / {update}:\n  " + "\n  ".join(problems)


@pytest.mark.parametrize("update", UPDATES)
@pytest.mark.parametrize("cuda", [True, False])
def test_update_reaches_the_drop_in_encoders(cuda, update):
    """model.py's wiring on Cora's 1433 raw features and the 50-wide layer (zero-padded inside the engine), the fixture's injected sets.
    cuda=True: table and weights on the device (the engine reads the Parameters); cuda=False: on the host (the Encoders keep device
    copies).  The `.data` calls are made on enc2 in one mode and on enc1 in the other: either Encoder of the pair must do."""
    g = load_golden("cora_bow_gcn_5_5")
    k1, k2 = int(g["k1"]), int(g["k2"])
    sets1 = sets_from_padded(g["layer1_nodes"], g["nbr1"], g["cnt1"])
    sets2 = sets_from_padded(g["seeds"], g["nbr2"], g["cnt2"])
    seeds = [int(s) for s in g["seeds"]]

    def modules(table, w1, w2):
        enc1, enc2 = build_modules(g, k1, k2, cuda, sets1, sets2)
        with torch.no_grad():
            enc1.features.weight.copy_(table)
            enc1.weight.copy_(w1)
            enc2.weight.copy_(w2)
        if cuda:
            enc2.to(DEV)
        return enc1, enc2

    def run(enc2):
        random.seed(5)
        with torch.no_grad():
            return enc2(seeds).detach().cpu().clone()

    table0, w10, w20 = full_table(g), torch.from_numpy(g["w1"]), torch.from_numpy(g["w2"])
    enc1, enc2 = modules(table0, w10, w20)
    assert enc2._can_fuse_two_hop()
    before = run(enc2)
    eng = enc2._engine
    assert eng is not None and eng._padded and eng.table.shape[1] == 1436 and eng.table is not enc1.features.weight
    gen = torch.Generator().manual_seed(9)
    read = np.array(sorted(set(g["nbr1"][np.arange(k1)[None, :] < g["cnt1"][:, None]].tolist())))
    rows = torch.from_numpy(np.concatenate([g["seeds"][:8], read[:: 3]]).astype(np.int64))
    rows = torch.unique(rows)
    new_rows = (torch.rand(len(rows), table0.shape[1], generator=gen) < 0.05).float() * torch.rand(len(rows), 1, generator=gen) * 3
    d1 = torch.randn(w10.shape, generator=gen) * float(w10.std()) * 0.5
    d2 = torch.randn(w20.shape, generator=gen) * float(w20.std()) * 0.5
    tw = enc1.features.weight
    if update == "table_inplace":
        with torch.no_grad():
            tw[rows.to(tw.device)] = new_rows.to(tw.device)
    elif update == "table_data":
        tw.data[rows.to(tw.device)] = new_rows.to(tw.device)
        (enc2 if cuda else enc1).refresh_features()
    elif update == "weights_inplace":
        with torch.no_grad():
            enc1.weight.add_(d1.to(enc1.weight.device))
            enc2.weight.add_(d2.to(enc2.weight.device))
    else:
        enc1.weight.data.add_(d1.to(enc1.weight.device))
        enc2.weight.data.add_(d2.to(enc2.weight.device))
        (enc1 if cuda else enc2).invalidate_weights()
    after = run(enc2)
    table1, w11, w21 = tw.detach().cpu().clone(), enc1.weight.detach().cpu().clone(), enc2.weight.detach().cpu().clone()
    want = run(modules(table1, w11, w21)[1])
    assert_close_rowmax(after, torch_two_hop(table1.double(), w11.double(), w21.double(), g).t(), rows_dim=1,
                        what=f"cuda={cuda} {update}: vs fp64")
    assert not _same(want, before), "the update changed nothing"
    assert _same(after, want), "output differs from freshly built modules on the updated tensors" + (" (= the stale output)" if _same(after, before) else "")
    assert _pads_are_zero(enc2._engine)


def test_a_sibling_made_before_the_first_forward_shares_the_slice_major_copy():
    """The smallest split layer 1 (512 seeds x fanout 15 + 512 = the 8192 frontier rows of sage_forward2_layout's threshold, d0 = 64):
    whether a sibling's layer 1 reads the slice-major copy must not depend on whether it was created before or after the parent's
    first forward, and after a table write the copy is refreshed once, in place, by whichever engine runs first."""
    graph = rmat_graph(12, 60_000, seed=3)
    d0, h1, h2, b, k1, k2 = 64, 32, 32, 512, 10, 15
    gen = torch.Generator().manual_seed(12)
    table = torch.randn(graph.num_nodes, d0, generator=gen).to(DEV)
    w1 = (torch.randn(h1, d0, generator=gen) / np.sqrt(d0)).to(DEV)
    w2 = (torch.randn(h2, h1, generator=gen) / np.sqrt(h1)).to(DEV)
    rng = np.random.default_rng(12)
    cand = np.nonzero(graph.degrees() > 0)[0]
    seeds = torch.from_numpy(rng.choice(cand, b, replace=False).astype(np.int32)).to(DEV)
    rowptr, col = graph.to(DEV)
    eng = TwoHopEngine(rowptr, col, table, w1, w2, k1, k2, max_batch=b)
    sib = eng.sibling()                                # before any forward
    assert eng.layout.layer1_split == 1 and sib.layout.layer1_split == 1
    before = eng.forward(seeds, seed=KEY).clone()
    sib_out = sib.forward(seeds, seed=KEY).clone()
    assert eng._table_sliced is not None and sib._table_sliced is eng._table_sliced
    ptr = eng._table_sliced.data_ptr()
    assert eng._model().table_sliced == ptr and sib._model().table_sliced == ptr
    assert torch.equal(sib_out, before)
    rows = torch.from_numpy(rng.choice(cand, 256, replace=False).astype(np.int64)).to(DEV)
    table[rows] = (torch.randn(len(rows), d0, generator=gen) * 2).to(DEV)
    sib_after = sib.forward(seeds, seed=KEY).clone()    # the sibling notices and refreshes the shared copy ...
    stamp = eng._tables.sliced_version
    eng_after = eng.forward(seeds, seed=KEY).clone()    # ... the parent finds it up to date
    assert eng._tables.sliced_version == stamp == table._version
    want = TwoHopEngine(rowptr, col, table, w1, w2, k1, k2, max_batch=b).forward(seeds, seed=KEY)
    assert not torch.equal(want, before), "the update changed nothing: it cannot tell a fresh copy from a stale one"
    assert torch.equal(sib_after, want) and torch.equal(eng_after, want)
    assert eng._table_sliced.data_ptr() == ptr and sib._table_sliced is eng._table_sliced
    assert eng._model().table_sliced == ptr and sib._model().table_sliced == ptr
