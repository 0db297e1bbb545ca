"""Alternating layer-1 streams (csrc/sage_pipe.hip, SAGE_PIPE_G_ALT): while stage D launches nothing, role G's calls for every odd
batch go to stream D's idle queue.  Same kernels, events, workspaces and arguments, so every output must equal the single forward's bit
for bit, with the knob on and off; `sage_pipe_alternate_count` says the path was taken.

The knob is read once per process, so each (knob, host threads) pair runs in ONE fresh child process (this file run as a script by
subprocess: a new process, never an exec).  The child runs every scenario at depth 2 and 4 and prints one JSON line of plain facts; the
tests below assert on them.  Knob "1" / "0" force the placement on / off; "" leaves it to the pipe, which takes it because
RolePipeline's default priorities put stream L above the layer-1 streams.  Six children in all, shared by every case.

Shape: the smallest at which the pipe takes the one-launch (phase-sliced) layer 1: d0 = 64, h1 = h2 = 32, k1 = 3, k2 = 15, batch = 512
gives max_s1 = 512 * 16 = 8192, the layer1_split threshold of sage_forward2_layout; a random graph of 2^12 nodes."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
D0, H1, H2, K1, K2, B, SCALE = 64, 32, 32, 3, 15, 512, 12
DEPTHS = (2, 4)


# ------------------------------------------------------------------------------------------------------------- the child process
def _scenarios(threads):
    import numpy as np
    import torch

    from sage355 import native, ops
    from sage355.engine import RolePipeline, TwoHopEngine
    from sage355.graph import rmat_graph

    dev = "cuda"
    graph = rmat_graph(SCALE, 60_000, seed=1)
    gen = torch.Generator().manual_seed(7)
    table = torch.randn(graph.num_nodes, D0, generator=gen).to(dev)
    w1 = (torch.randn(H1, D0, generator=gen) / 8).to(dev)
    w2 = (torch.randn(H2, H1, generator=gen) / 6).to(dev)
    rowptr, col = graph.to(dev)
    cand = np.nonzero(graph.degrees() > 0)[0]
    rs = np.random.default_rng(3)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]
    res = {"knob": os.environ.get("SAGE_PIPE_G_ALT", ""), "threads": threads, "depth": {}}
    for depth in DEPTHS:
        n = 2 * depth + 3
        seeds = torch.from_numpy(np.stack([rs.choice(cand, B, replace=False) for _ in range(n)]).astype(np.int32)).to(dev)
        keys = [500 + 10 * depth + i for i in range(n)]
        # the references, computed once and up front (no host work between the pipe's submits): W1, then W1 * 1.25, then that * 0.8
        wa = w1.clone()
        wb = wa.clone().mul_(1.25)
        wc = wb.clone().mul_(0.8)

        def reference(w):
            eng = TwoHopEngine(rowptr, col, table, w, w2, K1, K2, max_batch=B)
            return torch.stack([eng.forward(seeds[i], seed=keys[i]).clone() for i in range(n)])
        want, want_b, want_c = reference(wa), reference(wb), reference(wc)
        torch.cuda.synchronize()
        w1p = w1.clone()                                   # the pipe's own W1 tensor: written in place below
        pipe = RolePipeline(rowptr, col, table, w1p, w2, K1, K2, batch=B, depth=depth, threads=threads)
        e0 = pipe.engines[0]
        r = {"n": n}
        r["phase_form"] = bool(e0.layout.layer1_split == 1 and e0.layout.max_s1 == 8192 and ops.layer1_fused_supported(D0, H1, K1)
                               and e0._table_sliced is not None and e0._model().w1_prepared)
        # (a) n consecutive batches, no drain in between; which lane each took is read from the counters after every submit
        out = torch.zeros(n, B, H2, device=dev)
        express, expected_alt = [], 0
        for i in range(n):
            before = pipe.express_count
            pipe.submit(seeds[i], keys[i], out[i])
            express.append(pipe.express_count - before)
            expected_alt += 1 if (i % 2 == 1 and not express[-1]) else 0
        pipe.synchronize()
        r["express"], r["expected_alt"], r["alt"] = express, expected_alt, pipe.alternate_count
        r["equal"] = [bool(torch.equal(out[i], want[i])) for i in range(n)]
        # (b) the same again through submit_many (one host loop): batch indices n .. 2n - 1, n odd, so the parities are swapped per slot
        out.zero_()
        before_alt, before_exp = pipe.alternate_count, pipe.express_count
        pipe.submit_many(seeds, keys, out)
        pipe.synchronize()
        r["many_equal"] = bool(torch.equal(out, want))
        r["many_alt"], r["many_express"] = pipe.alternate_count - before_alt, pipe.express_count - before_exp
        r["many_odd"] = sum(1 for i in range(n, 2 * n) if i % 2 == 1)
        # (c) a weight update between two batches, the host never waiting: new bits from the very next batch on.  Batches 2n, 2n + 1
        # (even, odd) with the old W1; W1 is written in place on the current stream behind a join (the caller's side of the contract); then
        # 2n + 2, 2n + 3, 2n + 4; a second update, so that the first batch behind an update is an odd one too (2n + 5), then 2n + 6
        out.zero_()
        before_alt = pipe.alternate_count
        pipe.submit(seeds[0], keys[0], out[0])
        pipe.submit(seeds[1], keys[1], out[1])
        pipe.join()
        w1p.mul_(1.25)
        pipe.submit(seeds[2], keys[2], out[2])
        pipe.submit(seeds[3], keys[3], out[3])
        pipe.submit(seeds[4], keys[4], out[4])
        pipe.join()
        w1p.mul_(0.8)
        pipe.submit(seeds[0], keys[0], out[5])
        pipe.submit(seeds[1], keys[1], out[6])
        pipe.synchronize()
        r["update_old"] = bool(torch.equal(out[0], want[0]) and torch.equal(out[1], want[1]))
        r["update_new"] = [bool(torch.equal(out[i], want_b[i])) for i in (2, 3, 4)]
        r["update_differs"] = bool(not torch.equal(want_b[2], want[2]) and not torch.equal(want_c[0], want[0]))
        r["update_new_odd_first"] = [bool(torch.equal(out[5], want_c[0])), bool(torch.equal(out[6], want_c[1]))]
        r["update_alt"] = pipe.alternate_count - before_alt
        r["phase_form_after_update"] = bool(e0._model().w1_prepared)
        # (d) a profiled submit on an odd batch: the pair rides on the launch, whichever stream it took
        pipe.reset()                                        # everything is synchronised: indices restart at 0
        pairs = []
        for i in range(4):
            arr = (ctypes.c_void_p * 2)()
            for j in range(2):
                ev = ctypes.c_void_p()
                assert hip.hipEventCreate(ctypes.byref(ev)) == 0
                arr[j] = ev
            pairs.append(arr)
        before_alt = pipe.alternate_count
        lanes = []
        for i in range(4):
            before = pipe.express_count
            pipe.submit_profiled(seeds[i], keys[i], out[i], pairs[i])
            lanes.append(pipe.express_count - before)
        pipe.synchronize()
        torch.cuda.synchronize()
        ms = []
        for arr in pairs:
            v = ctypes.c_float(-1.0)
            rc = hip.hipEventElapsedTime(ctypes.byref(v), arr[0], arr[1])
            ms.append(v.value if rc == 0 else -1.0)
        r["profiled_ms"], r["profiled_express"], r["profiled_alt"] = ms, lanes, pipe.alternate_count - before_alt
        r["profiled_equal"] = bool(all(torch.equal(out[i], want_c[i]) for i in range(4)))
        # (e) a captured region: today's placement, alternate count unchanged, replays bit-identically
        cap_out = torch.zeros(n, B, H2, device=dev)
        before_alt = pipe.alternate_count
        g, stream = pipe.capture(seeds, keys, cap_out)
        torch.cuda.synchronize()
        replays = []
        for _ in range(2):
            cap_out.zero_()
            with torch.cuda.stream(stream):
                g.replay()
            torch.cuda.synchronize()
            replays.append(cap_out.clone())
        r["capture_equal"] = bool(all(torch.equal(rep, want_c) for rep in replays))
        r["capture_alt"] = pipe.alternate_count - before_alt
        # and eager submission afterwards alternates again
        out.zero_()
        before_alt, before_exp = pipe.alternate_count, pipe.express_count
        pipe.submit_many(seeds, keys, out)
        pipe.synchronize()
        r["after_capture_equal"] = bool(torch.equal(out, want_c))
        r["after_capture_alt"], r["after_capture_express"] = pipe.alternate_count - before_alt, pipe.express_count - before_exp
        res["depth"][str(depth)] = r
        del g, pipe
    return res


if __name__ == "__main__":
    _repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (_repo, os.path.join(_repo, "graphsage-simple_amd")):
        sys.path.insert(0, _p)
    print("RESULT " + json.dumps(_scenarios(sys.argv[1] == "1")))
    sys.exit(0)


# ------------------------------------------------------------------------------------------------------------------- the tests
@functools.lru_cache(maxsize=None)
def child(knob, threads):
    env = dict(os.environ, SAGE_PIPE_G_ALT=knob)
    if knob == "":
        del env["SAGE_PIPE_G_ALT"]                         # unset: the pipe's streams decide (RolePipeline's default priorities: taken)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "1" if threads else "0"], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, f"child (SAGE_PIPE_G_ALT={knob}, threads={threads}) exit {p.returncode}:\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    res = json.loads(line[len("RESULT "):])
    assert res["knob"] == knob and res["threads"] == threads
    return res


CASES = [(knob, threads, depth) for knob in ("1", "0", "") for threads in (False, True) for depth in DEPTHS]


@pytest.mark.parametrize("knob,threads,depth", CASES)
def test_consecutive_batches_are_bit_identical_and_the_count_says_which_stream(knob, threads, depth):
    r = child(knob, threads)["depth"][str(depth)]
    print(r)
    assert r["phase_form"], "the one-launch layer 1 is not this shape's form: the test would not reach the alternation"
    assert r["n"] == 2 * depth + 3
    assert all(r["equal"]), r["equal"]
    assert r["express"][0] == 1, "the first batch of an idle pipe takes the express lane"
    assert r["alt"] == (r["expected_alt"] if knob != "0" else 0), (r["alt"], r["expected_alt"], r["express"])
    if knob != "0":
        assert r["expected_alt"] >= 1, "every odd batch found the pipe idle: the alternation was never reached"
    assert r["many_equal"]
    if knob != "0":
        assert r["many_odd"] - r["many_express"] <= r["many_alt"] <= r["many_odd"], r
    else:
        assert r["many_alt"] == 0


@pytest.mark.parametrize("knob,threads,depth", CASES)
def test_weight_update_reaches_the_very_next_batch_on_either_stream(knob, threads, depth):
    r = child(knob, threads)["depth"][str(depth)]
    assert r["update_differs"], "the changed W1 must change the output, or the case shows nothing"
    assert r["update_old"], "batches submitted before the update must carry the old weights' bits"
    assert all(r["update_new"]), r["update_new"]
    assert all(r["update_new_odd_first"]), r["update_new_odd_first"]
    assert r["phase_form_after_update"]
    assert (r["update_alt"] >= 1) if knob != "0" else (r["update_alt"] == 0)      # batch 2n + 1 follows 2n at once: it is never express


@pytest.mark.parametrize("knob,threads,depth", CASES)
def test_profiled_submit_on_an_odd_batch_returns_a_positive_interval(knob, threads, depth):
    r = child(knob, threads)["depth"][str(depth)]
    print(r["profiled_ms"], r["profiled_express"], r["profiled_alt"])
    assert all(ms > 0 for ms in r["profiled_ms"]), r["profiled_ms"]
    assert r["profiled_equal"]
    odd_not_express = sum(1 for i in (1, 3) if not r["profiled_express"][i])
    assert r["profiled_alt"] == (odd_not_express if knob != "0" else 0)


@pytest.mark.parametrize("knob,threads,depth", CASES)
def test_captured_region_keeps_its_placement_and_replays_bit_identically(knob, threads, depth):
    r = child(knob, threads)["depth"][str(depth)]
    assert r["capture_equal"]
    assert r["capture_alt"] == 0, "no alternation inside a stream capture"
    assert r["after_capture_equal"]
    if knob != "0":
        odd = r["n"] // 2
        assert max(1, odd - r["after_capture_express"]) <= r["after_capture_alt"] <= odd, r
    else:
        assert r["after_capture_alt"] == 0
