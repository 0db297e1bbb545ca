"""Inner sampler in front of layer 1 (csrc/sage_pipe.hip, SAGE_PIPE_SI_WITH_L1): wherever the pipe alternates its layer-1 streams, role S
launches only the outer hop and role G launches the inner hop and then layer 1 on the batch's layer-1 stream.  Same kernels, events,
workspaces and arguments, so every output must equal the single forward's bit for bit, with the knob on, off and unset;
`sage_pipe_inner_with_layer1_count` says the cut was taken.

The knobs are read once per process, so each (knobs, host threads) pair runs in ONE fresh child process (this file run as a script by
subprocess: a new process, never an exec).  A child runs every scenario at depths 1 to 4 with 2 * depth + 3 batches each (an odd count:
every slot sees both parities and both layer-1 streams) and prints one JSON line of plain facts; the tests below assert on them.

Shape: the smallest at which the pipe takes the one-launch (phase-sliced) layer 1: d0 = 64, h1 = h2 = 32, k1 = 3, k2 = 15, batch = 512
gives max_s1 = 512 * 16 = 8192, the layer1_split threshold of sage_forward2_layout; a random graph of 2^12 nodes, plus 512 isolated
nodes behind them for the batch whose frontier stays empty."""
import ctypes
import functools
import json
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu
D0, H1, H2, K1, K2, B, SCALE = 64, 32, 32, 3, 15, 512, 12
DEPTHS = (1, 2, 3, 4)
KNOB, ALT = "SAGE_PIPE_SI_WITH_L1", "SAGE_PIPE_G_ALT"


# ------------------------------------------------------------------------------------------------------------- the child process
def _bits_equal(a, b):
    import torch
    return bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))      # NaN-proof: the bits


def _scenarios(threads, everything):
    import numpy as np
    import torch

    from sage355 import ops
    from sage355.engine import RolePipeline, TwoHopEngine, pretransform_table
    from sage355.graph import CSRGraph, rmat_graph

    dev = "cuda"
    g0 = rmat_graph(SCALE, 60_000, seed=1)
    # B isolated nodes behind the generated ones: rows of length 0, named by no edge
    graph = CSRGraph(np.concatenate([g0.rowptr, np.full(B, g0.rowptr[-1], dtype=g0.rowptr.dtype)]), g0.col, g0.num_nodes + B)
    deg = graph.degrees()
    gen = torch.Generator().manual_seed(7)
    table = torch.randn(graph.num_nodes, D0, generator=gen).to(dev)
    w1 = (torch.randn(H1, D0, generator=gen) / 8).to(dev)
    w2 = (torch.randn(H2, H1, generator=gen) / 6).to(dev)
    rowptr, col = graph.to(dev)
    cand = np.nonzero(deg > 0)[0]
    isolated = np.arange(g0.num_nodes, graph.num_nodes)
    rs = np.random.default_rng(3)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]
    res = {"knob": os.environ.get(KNOB, ""), "alt_knob": os.environ.get(ALT, ""), "threads": threads, "depth": {}}

    def counted_submits(pipe, seeds, keys, out, idx, index0=0):
        """submit() of batches idx in turn -> per batch: took the express lane, and (pipe index is odd and not express)"""
        express, odd = [], 0
        for j, i in enumerate(idx):
            before = pipe.express_count
            pipe.submit(seeds[i], keys[i], out[j])
            express.append(pipe.express_count - before)
            odd += 1 if ((index0 + j) % 2 == 1 and not express[-1]) else 0
        return express, odd

    for depth in DEPTHS:
        n = 2 * depth + 3
        seeds_np = np.stack([rs.choice(cand, B, replace=False) for _ in range(n)])
        seeds = torch.from_numpy(seeds_np.astype(np.int32)).to(dev)
        keys = [700 + 10 * depth + i for i in range(n)]
        wa = w1.clone()
        wb = wa.clone().mul_(1.25)
        wc = wb.clone().mul_(0.8)

        def reference(w, **kw):
            eng = TwoHopEngine(rowptr, col, table, w, w2, K1, K2, max_batch=B, **kw)
            return torch.stack([eng.forward(seeds[i], seed=keys[i]).clone() for i in range(n)]), eng
        want, _ = reference(wa)
        r = {"n": n}
        w1p = w1.clone()                                   # the pipe's own W1 tensor: written in place below
        pipe = RolePipeline(rowptr, col, table, w1p, w2, K1, K2, batch=B, depth=depth, threads=threads)
        e0 = pipe.engines[0]
        r["phase_form"] = bool(e0.layout.layer1_split == 1 and e0.layout.max_s1 == 8192 and ops.layer1_fused_supported(D0, H1, K1)
                               and e0._table_sliced is not None and e0._model().w1_prepared)
        # (1) n consecutive batches through submit, then through submit_many (indices n .. 2n - 1, n odd: the parities swap per slot)
        out = torch.zeros(n, B, H2, device=dev)
        r["express"], r["expected_alt"] = counted_submits(pipe, seeds, keys, out, range(n))
        pipe.synchronize()
        r["inner"], r["alt"] = pipe.inner_with_layer1_count, pipe.alternate_count
        r["equal"] = [_bits_equal(out[i], want[i]) for i in range(n)]
        out.zero_()
        b_in, b_alt, b_exp = pipe.inner_with_layer1_count, pipe.alternate_count, pipe.express_count
        pipe.submit_many(seeds, keys, out)
        pipe.synchronize()
        r["many_equal"] = _bits_equal(out, want)
        r["many_inner"], r["many_alt"], r["many_express"] = (pipe.inner_with_layer1_count - b_in, pipe.alternate_count - b_alt,
                                                             pipe.express_count - b_exp)
        r["many_odd"] = sum(1 for i in range(n, 2 * n) if i % 2 == 1)
        if not everything:
            res["depth"][str(depth)] = r
            del pipe
            continue
        want_b, _ = reference(wb)
        want_c, _ = reference(wc)
        torch.cuda.synchronize()
        # (3) a weight update between two batches, the host never waiting: W1 is written in place on the current stream behind a join
        # (the caller's side of the contract).  Indices 2n, 2n + 1 with the old W1 | 2n + 2 .. 2n + 4 | a second update, so that the
        # first batch behind an update is of the other parity too: 2n + 5, 2n + 6
        upd = torch.zeros(7, B, H2, device=dev)
        b_in, b_exp = pipe.inner_with_layer1_count, pipe.express_count
        pipe.submit(seeds[0], keys[0], upd[0])
        pipe.submit(seeds[1], keys[1], upd[1])
        pipe.join()
        w1p.mul_(1.25)
        pipe.submit(seeds[2], keys[2], upd[2])
        pipe.submit(seeds[3], keys[3], upd[3])
        pipe.submit(seeds[4], keys[4], upd[4])
        pipe.join()
        w1p.mul_(0.8)
        pipe.submit(seeds[0], keys[0], upd[5])
        pipe.submit(seeds[1], keys[1], upd[6])
        pipe.synchronize()
        r["update_old"] = bool(_bits_equal(upd[0], want[0]) and _bits_equal(upd[1], want[1]))
        r["update_new"] = [_bits_equal(upd[i], want_b[i]) for i in (2, 3, 4)]
        r["update_differs"] = bool(not _bits_equal(want_b[2], want[2]) and not _bits_equal(want_c[0], want[0]))
        r["update_new_odd_first"] = [_bits_equal(upd[5], want_c[0]), _bits_equal(upd[6], want_c[1])]
        r["update_inner"], r["update_express"] = pipe.inner_with_layer1_count - b_in, pipe.express_count - b_exp
        r["phase_form_after_update"] = bool(e0._model().w1_prepared)
        # (4) profiled submits on even and odd batches: the pair is positive and shorter than the batch's stay in the pipe
        pipe.reset()                                        # everything is synchronised: indices restart at 0
        pairs = []
        for i in range(4):
            arr = (ctypes.c_void_p * 2)()
            for j in range(2):
                ev = ctypes.c_void_p()
                assert hip.hipEventCreate(ctypes.byref(ev)) == 0
                arr[j] = ev
            pairs.append(arr)
        b_in, lanes, t_submit = pipe.inner_with_layer1_count, [], []
        for i in range(4):
            before = pipe.express_count
            t_submit.append(time.perf_counter())
            pipe.submit_profiled(seeds[i], keys[i], out[i], pairs[i])
            lanes.append(pipe.express_count - before)
        pipe.synchronize()
        torch.cuda.synchronize()
        t_done = time.perf_counter()                        # every batch has completed by now: an upper bound of each one's completion
        ms = []
        for arr in pairs:
            v = ctypes.c_float(-1.0)
            rc = hip.hipEventElapsedTime(ctypes.byref(v), arr[0], arr[1])
            ms.append(v.value if rc == 0 else -1.0)
        r["profiled_ms"], r["profiled_express"], r["profiled_inner"] = ms, lanes, pipe.inner_with_layer1_count - b_in
        r["profiled_stay_ms"] = [(t_done - t) * 1e3 for t in t_submit]
        r["profiled_equal"] = bool(all(_bits_equal(out[i], want_c[i]) for i in range(4)))
        # (8) after reset() the indices restart: the same three batches again count as the first three did
        pipe.reset()
        b_in, b_alt = pipe.inner_with_layer1_count, pipe.alternate_count
        ex, odd = counted_submits(pipe, seeds, keys, out, range(3))
        pipe.synchronize()
        r["reset_express"], r["reset_odd"] = ex, odd
        r["reset_inner"], r["reset_alt"] = pipe.inner_with_layer1_count - b_in, pipe.alternate_count - b_alt
        r["reset_equal"] = bool(all(_bits_equal(out[i], want_c[i]) for i in range(3)))
        # (5) an empty frontier between two ordinary batches: every seed of the middle batch is an isolated node
        iso = torch.from_numpy(rs.choice(isolated, B, replace=False).astype(np.int32)).to(dev)
        r["empty_degrees_zero"] = bool((deg[iso.cpu().numpy()] == 0).all())
        r["neighbours_degrees_positive"] = bool((deg[seeds_np[0]] > 0).all() and (deg[seeds_np[1]] > 0).all())
        eng_c = TwoHopEngine(rowptr, col, table, wc, w2, K1, K2, max_batch=B)
        want_empty = eng_c.forward(iso, seed=99).clone()
        r["empty_n_s1"] = int(eng_c.intermediates()["n_s1"])
        out.zero_().add_(7.0)                               # not zero: a launch that wrote nothing would show
        b_in = pipe.inner_with_layer1_count
        ex = []
        for j, (sd, key) in enumerate(((seeds[0], keys[0]), (iso, 99), (seeds[1], keys[1]))):
            before = pipe.express_count
            pipe.submit(sd, key, out[j])
            ex.append(pipe.express_count - before)
        pipe.synchronize()
        r["empty_express"], r["empty_inner"] = ex, pipe.inner_with_layer1_count - b_in
        r["empty_equal"] = _bits_equal(out[1], want_empty)
        r["empty_reference_is_zero"] = bool((want_empty == 0).all())
        r["empty_zero_where_reference_zero"] = bool((out[1][want_empty == 0] == 0).all())
        r["empty_neighbours_equal"] = bool(_bits_equal(out[0], want_c[0]) and _bits_equal(out[2], want_c[1]))
        # (7) capture() of 2 * depth + 1 batches: today's cut inside, the count does not move, the replay equals the eager outputs
        m = 2 * depth + 1
        cap_out = torch.zeros(m, B, H2, device=dev)
        b_in = pipe.inner_with_layer1_count
        g, stream = pipe.capture(seeds[:m], keys[:m], cap_out)
        torch.cuda.synchronize()
        replays = []
        for _ in range(2):
            cap_out.zero_()
            with torch.cuda.stream(stream):
                g.replay()
            torch.cuda.synchronize()
            replays.append(cap_out.clone())
        r["capture_equal"] = bool(all(_bits_equal(rep, want_c[:m]) for rep in replays))
        r["capture_inner"] = pipe.inner_with_layer1_count - b_in
        out.zero_()
        b_in, b_exp = pipe.inner_with_layer1_count, pipe.express_count
        pipe.submit_many(seeds, keys, out)
        pipe.synchronize()
        r["after_capture_equal"] = _bits_equal(out, want_c)
        r["after_capture_inner"], r["after_capture_express"] = pipe.inner_with_layer1_count - b_in, pipe.express_count - b_exp
        del g, pipe
        # (6) the other encoder forms, n consecutive batches each
        forms = {}
        w1sq = (torch.randn(2 * H1, D0, generator=torch.Generator().manual_seed(11)) / 8).to(dev)          # [64, 64]: Y is 64 wide
        w2sq = (torch.randn(H2, 2 * H1, generator=torch.Generator().manual_seed(12)) / 6).to(dev)
        y, eye = pretransform_table(table, w1sq)
        w1cat = (torch.randn(H1, 2 * D0, generator=torch.Generator().manual_seed(13)) / 8).to(dev)
        for name, args, kw in (("pretransformed", (y, eye, w2sq), {}), ("concat", (table, w1cat, w2sq), {"concat": True}),
                               ("self_loop", (table, w1, w2), {"agg_self_loop": True})):
            eng = TwoHopEngine(rowptr, col, *args, K1, K2, max_batch=B, **kw)
            ref = torch.stack([eng.forward(seeds[i], seed=keys[i]).clone() for i in range(n)])
            fp = RolePipeline(rowptr, col, *args, K1, K2, batch=B, depth=depth, threads=threads, **kw)
            fo = torch.zeros(n, B, H2, device=dev)
            f = {}
            f["express"], f["odd"] = counted_submits(fp, seeds, keys, fo, range(n))
            fp.synchronize()
            f["inner"], f["alt"] = fp.inner_with_layer1_count, fp.alternate_count
            f["equal"] = bool(all(_bits_equal(fo[i], ref[i]) for i in range(n)))
            fe = fp.engines[0]
            f["split"], f["identity"], f["max_s1"] = int(fe.layout.layer1_split), int(fe._model().w1_is_identity), int(fe.layout.max_s1)
            forms[name] = f
            del fp
        r["forms"] = forms
        res["depth"][str(depth)] = r
    return res


if __name__ == "__main__":
    _repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (_repo, os.path.join(_repo, "graphsage-simple_amd")):
        sys.path.insert(0, _p)
    print("RESULT " + json.dumps(_scenarios(sys.argv[1] == "1", sys.argv[2] == "1")))
    sys.exit(0)


# ------------------------------------------------------------------------------------------------------------------- the tests
@functools.lru_cache(maxsize=None)
def child(knob, threads, alt_knob=""):
    env = dict(os.environ)
    for name, v in ((KNOB, knob), (ALT, alt_knob)):
        env.pop(name, None)                                 # unset: the pipe decides
        if v != "":
            env[name] = v
    everything = alt_knob == ""                             # the child without alternation runs the consecutive submits only
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "1" if threads else "0", "1" if everything else "0"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, f"child ({KNOB}={knob}, {ALT}={alt_knob}, threads={threads}) exit {p.returncode}:\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    res = json.loads(line[len("RESULT "):])
    assert res["knob"] == knob and res["alt_knob"] == alt_knob and res["threads"] == threads
    return res


CASES = [(knob, threads, depth) for knob in ("1", "0", "") for threads in (False, True) for depth in DEPTHS]


@pytest.mark.parametrize("knob,threads,depth", CASES)
def test_consecutive_submits_are_bit_identical_and_the_count_says_which_cut(knob, threads, depth):
    r = child(knob, threads)["depth"][str(depth)]
    print(r)
    assert r["phase_form"], "the one-launch layer 1 is not this shape's form: the test would not reach the placement"
    assert r["n"] == 2 * depth + 3
    assert all(r["equal"]), r["equal"]
    assert r["express"][0] == 1, "the first batch of an idle pipe takes the express lane"
    not_express = r["n"] - sum(r["express"])
    assert not_express >= 1, "every batch found the pipe idle: the role streams were never reached"
    assert r["inner"] == (not_express if knob != "0" else 0), (r["inner"], r["express"])
    assert r["alt"] == r["expected_alt"], "the alternation does not depend on this knob"
    assert r["many_equal"]
    assert r["many_inner"] == (r["n"] - r["many_express"] if knob != "0" else 0), r
    assert r["many_odd"] - r["many_express"] <= r["many_alt"] <= r["many_odd"], r


@pytest.mark.parametrize("threads", [False, True])
@pytest.mark.parametrize("depth", DEPTHS)
def test_forcing_it_on_without_the_alternation_changes_nothing(threads, depth):
    r = child("1", threads, "0")["depth"][str(depth)]
    assert r["phase_form"]
    assert all(r["equal"]) and r["many_equal"]
    assert r["inner"] == 0 and r["many_inner"] == 0 and r["alt"] == 0 and r["many_alt"] == 0, r


@pytest.mark.parametrize("knob,threads,depth", CASES)
def test_weight_update_between_an_even_and_an_odd_batch(knob, threads, depth):
    r = child(knob, threads)["depth"][str(depth)]
    assert r["update_differs"], "the changed W1 must change the output, or the case shows nothing"
    assert r["update_old"], "batches submitted before the update must carry the old weights' bits"
    assert all(r["update_new"]), r["update_new"]
    assert all(r["update_new_odd_first"]), r["update_new_odd_first"]
    assert r["phase_form_after_update"]
    assert r["update_inner"] == (7 - r["update_express"] if knob != "0" else 0), r


@pytest.mark.parametrize("knob,threads,depth", CASES)
def test_profiled_pair_rides_on_layer_1(knob, threads, depth):
    r = child(knob, threads)["depth"][str(depth)]
    print(r["profiled_ms"], r["profiled_stay_ms"], r["profiled_express"])
    assert all(ms > 0 for ms in r["profiled_ms"]), r["profiled_ms"]
    assert all(ms < stay for ms, stay in zip(r["profiled_ms"], r["profiled_stay_ms"])), (r["profiled_ms"], r["profiled_stay_ms"])
    assert r["profiled_equal"]
    assert r["profiled_inner"] == (4 - sum(r["profiled_express"]) if knob != "0" else 0)


@pytest.mark.parametrize("knob,threads,depth", CASES)
def test_empty_frontier_between_two_ordinary_batches(knob, threads, depth):
    r = child(knob, threads)["depth"][str(depth)]
    assert r["empty_degrees_zero"] and r["neighbours_degrees_positive"]
    assert r["empty_n_s1"] == 0, "the single forward's frontier is not empty: the case shows nothing"
    assert r["empty_equal"] and r["empty_zero_where_reference_zero"], r
    assert r["empty_neighbours_equal"]
    assert r["empty_inner"] == (3 - sum(r["empty_express"]) if knob != "0" else 0)


@pytest.mark.parametrize("knob,threads,depth", CASES)
def test_other_encoder_forms(knob, threads, depth):
    forms = child(knob, threads)["depth"][str(depth)]["forms"]
    print(forms)
    for name, f in forms.items():
        assert f["equal"], name
        n = 2 * depth + 3
        takes = name != "concat"                            # stage D is not empty for the concat encoder
        assert f["inner"] == (n - sum(f["express"]) if (takes and knob != "0") else 0), (name, f)
        assert f["alt"] == (f["odd"] if takes else 0), (name, f)
    assert forms["pretransformed"]["identity"] == 1 and forms["pretransformed"]["split"] == 1, "not the gather-only layer 1"


@pytest.mark.parametrize("knob,threads,depth", CASES)
def test_capture_keeps_the_old_cut_and_replays_bit_identically(knob, threads, depth):
    r = child(knob, threads)["depth"][str(depth)]
    assert r["capture_equal"]
    assert r["capture_inner"] == 0, "inside a stream capture the cut stays as it was"
    assert r["after_capture_equal"]
    assert r["after_capture_inner"] == (r["n"] - r["after_capture_express"] if knob != "0" else 0), r


@pytest.mark.parametrize("knob,threads,depth", CASES)
def test_reset_restarts_the_indices(knob, threads, depth):
    r = child(knob, threads)["depth"][str(depth)]
    assert r["reset_equal"]
    assert r["reset_inner"] == (3 - sum(r["reset_express"]) if knob != "0" else 0), r
    assert r["reset_alt"] == r["reset_odd"], r
