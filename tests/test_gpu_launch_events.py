"""The events a launch carries as its own start / stop events (csrc/sage_internal.h, sage_launch_events_t): the profiled forward's ten stage
events, the profiled submit's gather pair in both lanes of the role pipeline, and the stream-coincidence path where records are skipped.
Only `bench.py --full` used these paths before."""
import ctypes

import numpy as np
import pytest
import torch

from sage355.engine import RolePipeline, TwoHopEngine
from sage355.graph import rmat_graph

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, K1, K2 = 512, 15, 25           # the smoke test's problem: max_s1 = 13 312 >= 8192, so a 256-wide layer 1 takes the split form
KEYS = [42, 43, 44, 45]


class Hip:
    def __init__(self):
        self.hip = ctypes.CDLL("libamdhip64.so")
        self.hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]
        self.hip.hipEventDestroy.argtypes = [ctypes.c_void_p]
        self.made = []

    def events(self, n):
        arr = (ctypes.c_void_p * n)()
        for i in range(n):
            ev = ctypes.c_void_p()
            assert self.hip.hipEventCreate(ctypes.byref(ev)) == 0
            arr[i] = ev
            self.made.append(ev)
        return arr

    def elapsed_ms(self, a, b):
        ms = ctypes.c_float(-1.0)
        rc = self.hip.hipEventElapsedTime(ctypes.byref(ms), a, b)
        assert rc == 0, f"hipEventElapsedTime -> {rc}"
        return ms.value

    def destroy(self):
        for ev in self.made:
            self.hip.hipEventDestroy(ev)
        self.made = []


@pytest.fixture()
def hip():
    h = Hip()
    yield h
    torch.cuda.synchronize()
    h.destroy()


def _problem(d0, h1, h2=64, concat=False):
    g = rmat_graph(12, 60_000, seed=1)
    gen = torch.Generator().manual_seed(0)
    table = torch.randn(g.num_nodes, d0, generator=gen)
    w1 = torch.randn(h1, d0 * (2 if concat else 1), generator=gen) / 16
    w2 = torch.randn(h2, h1 * (2 if concat else 1), generator=gen) / 11
    cand = np.nonzero(g.degrees() > 0)[0]
    rs = np.random.default_rng(0)
    seeds = torch.from_numpy(np.stack([rs.choice(cand, B, replace=False) for _ in KEYS]).astype(np.int32)).to(DEV)
    rowptr, col = g.to(DEV)
    return (rowptr, col, table.to(DEV), w1.to(DEV), w2.to(DEV), K1, K2), seeds


@pytest.fixture(scope="module")
def split_problem():
    """The gcn problem, and the single forward's output of every batch: the reference of the pipeline tests (computed once, never written)."""
    args, seeds = _problem(256, 128)
    eng = TwoHopEngine(*args, max_batch=B)
    assert eng.layout.layer1_split
    want = torch.stack([eng.forward(seeds[i], seed=KEYS[i]).clone() for i in range(len(KEYS))])
    return args, seeds, want


@pytest.mark.parametrize("case", ["gcn_phase_sliced", "gcn_keep_means", "concat", "one_launch_layer1"])
def test_profiled_forward_records_all_ten_events_and_changes_no_bit(case, hip):
    """TwoHopEngine.forward(stage_events=...): events 4 / 5 are the gather launch's own start / stop events when layer 1 takes the
    phase-sliced or a column-sliced form (gcn; gcn with the means kept = gather + contraction; concat) and marker records around an
    empty gather stage when layer 1 is one launch.  Either way every stage pair, and the pairs across two stages, can be read back."""
    if case == "one_launch_layer1":
        args, seeds = _problem(32, 32)
    else:
        args, seeds = _problem(256, 128, concat=case == "concat")
    eng = TwoHopEngine(*args, max_batch=B, concat=case == "concat")
    assert bool(eng.layout.layer1_split) == (case != "one_launch_layer1")
    eng.keep_means = case == "gcn_keep_means"
    want = eng.forward(seeds[0], seed=KEYS[0]).clone()
    ev = hip.events(10)
    got = eng.forward(seeds[0], seed=KEYS[0], stage_events=ev)
    torch.cuda.synchronize()
    for a, b in [(0, 1), (2, 3), (4, 5), (6, 7), (8, 9), (1, 2), (7, 8)]:
        ms = hip.elapsed_ms(ev[a], ev[b])
        print(f"{case}: events ({a}, {b}) {ms * 1e3:.1f} us")
        assert ms >= 0, (a, b, ms)
    assert torch.equal(got, want)


@pytest.mark.parametrize("threads", [False, True])
def test_profiled_submit_times_the_gather_in_both_lanes(threads, split_problem, hip):
    """RolePipeline.submit_profiled: the caller's pair rides on the layer-1 gather launch, in the express lane (the idle pipe's batch) and
    on role stream G (batches that find the pipe busy), and the role's hand-off event is then recorded behind the launch."""
    args, seeds, want = split_problem
    n = len(KEYS)
    pipe = RolePipeline(*args, batch=B, depth=2, threads=threads)
    assert pipe.engines[0].layout.layer1_split
    out = torch.zeros(n + 1, B, want.shape[2], device=DEV)
    pairs = [hip.events(2) for _ in range(n + 1)]
    count = pipe.express_count
    pipe.submit_profiled(seeds[0], KEYS[0], out[n], pairs[n])
    pipe.synchronize()
    assert pipe.express_count == count + 1
    for i in range(n):
        pipe.submit_profiled(seeds[i], KEYS[i], out[i], pairs[i])
    pipe.synchronize()
    torch.cuda.synchronize()
    for i, pair in enumerate(pairs):
        ms = hip.elapsed_ms(pair[0], pair[1])
        print(f"threads={threads}: gather of submit {i} {ms * 1e3:.1f} us")
        assert ms > 0, (i, ms)
    assert torch.equal(out[:n], want) and torch.equal(out[n], want[0])


def test_shared_role_streams_skip_records_and_change_no_bit(split_problem):
    """roles="SGDD": D and L share a stream, so D's hand-off is stream order -- no tail event, no record."""
    args, seeds, want = split_problem
    n = len(KEYS)
    pipe = RolePipeline(*args, batch=B, depth=2, roles="SGDD")
    out = torch.zeros(n, B, want.shape[2], device=DEV)
    for i in range(n):
        pipe.submit(seeds[i], KEYS[i], out[i])
    pipe.synchronize()
    assert torch.equal(out, want)
