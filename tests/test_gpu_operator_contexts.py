"""Every per-step operator (the cases of tests/contexts.py) outside the one execution context the per-kernel tests use -- device 0,
the default stream, eagerly:

a. on a fresh side stream, behind a delay, with the real contents written on that stream just before the call: a launch, a sort or a
   workspace step that went to another stream would read the decoy contents or a stale workspace.  One negative control shows that
   the harness sees exactly that.
b. with torch's synchronisation debug mode on "error": a per-step wrapper reads nothing back.
c. captured into a graph and replayed on three sets of contents: a launch size or a host value baked in from device data would show.
d. on a second GPU (skipped where there is one): the bits of device 0; and tensors of a device that is not the current one are refused.

Expected values are the operator's own bits on the default stream (the per-kernel tests own the values); gather_mean_backward, whose
fp32 atomics fix no order, is judged against fp64 with the bound of tests/test_gpu_backward_kernels.py in every context."""
import time

import pytest
import torch

import contexts
from sage355 import native, ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
DELAY_TARGET_MS = 10.0            # at least 5 ms is asked for; not derived: it only has to outlast the host's enqueue of one call
SIDE_STREAMS = 4                  # consecutive pool streams a case runs on: as many as a process has hardware queues by default


def _snap(outs):
    """Device copies of a call's outputs, on the current stream"""
    return [None if t is None else t.clone() for t in outs]


def _host(outs):
    return [None if t is None else t.cpu() for t in outs]


def _run(st, v):
    """Contents v, poisoned outputs and workspaces, one eager call on the current stream, synchronised -> CPU outputs"""
    st.fill(v)
    st.poison()
    got = _snap(st.call())
    torch.cuda.synchronize()
    return _host(got)


class Delay:
    """A chain of torch.mm on one stream, sized once: the smallest power-of-two number of 4096^3 products that takes DELAY_TARGET_MS
    by device events."""

    def __init__(self):
        self.a = torch.full((4096, 4096), 1.0 / 4096, device=DEV)
        self.b, self.c = torch.empty_like(self.a), torch.empty_like(self.a)
        self.reps = 1
        self.run()                                        # the BLAS library's first call
        torch.cuda.synchronize()
        while True:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            self.run()
            t1.record()
            torch.cuda.synchronize()
            self.ms = t0.elapsed_time(t1)
            if self.ms >= DELAY_TARGET_MS or self.reps >= 4096:
                break
            self.reps *= 2
        print(f"delay: {self.reps} products of 4096^3, {self.ms:.2f} ms by device events")

    def run(self):
        src, dst = self.a, self.b
        for _ in range(self.reps):                        # each product reads the one before: a chain
            torch.mm(src, self.a, out=dst)
            src, dst = dst, (self.c if dst is self.b else self.b)


@pytest.fixture(scope="module")
def delay():
    d = Delay()
    assert d.ms >= 5.0, f"the delay chain takes {d.ms:.2f} ms"
    return d


@pytest.fixture(scope="module")
def states():
    """name -> the case's State on device 0, built once per module"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = contexts.BY_NAME[name].build(DEV)
            torch.cuda.synchronize()
        return made[name]
    return get


def _behind_the_delay(st, delay, call_stream=None):
    """On a fresh stream s: the delay, the real contents, the call (on call_stream when given: a stream that does not wait for s), a copy
    of the outputs.  The inputs hold the decoy and the outputs sentinels before.  -> (CPU outputs, was the delay's event still
    pending when the call had returned, host milliseconds of the call)"""
    st.fill(1)
    st.poison()
    torch.cuda.synchronize()
    s = torch.cuda.Stream(DEV)
    behind = torch.cuda.Event()
    with torch.cuda.stream(s):
        delay.run()
        behind.record(s)
        st.fill(0)
        t0 = time.perf_counter()
        if call_stream is None:
            outs = st.call()
        else:
            with torch.cuda.stream(call_stream):
                outs = st.call()
        ms = (time.perf_counter() - t0) * 1e3
        pending = not behind.query()
        with torch.cuda.stream(call_stream if call_stream is not None else s):
            got = _snap(outs)
    s.synchronize()
    torch.cuda.synchronize()
    return _host(got), pending, ms


# ---------------------------------------------------------------------------------------------------------------- a. side stream
@pytest.mark.parametrize("name", contexts.NAMES)
def test_on_a_side_stream_behind_a_delay(states, delay, name):
    """On SIDE_STREAMS consecutive streams of torch's pool, one after the other: a step that strays to another stream (stream 0, say)
    goes unseen from a side stream that shares its hardware queue, which runs them in order by accident; consecutive streams are
    spread over the process's queues (four by default), so a stray step shares a queue with one of them at the most."""
    st = states(name)
    want = _run(st, 0)
    misses = []
    for i in range(SIDE_STREAMS):
        got, pending, ms = _behind_the_delay(st, delay)
        print(f"{name}, stream {i}: delay {delay.ms:.2f} ms, the call's enqueue {ms:.3f} ms, delay pending when the call returned: {pending}")
        assert pending, (f"inconclusive: the {delay.ms:.2f} ms delay had run out when the call returned after {ms:.3f} ms -- lengthen the "
                         "chain (DELAY_TARGET_MS); this says nothing about the operator")
        miss = st.verdict(0, got, want)
        if miss is not None:
            misses.append(f"stream {i}: {miss}")
    assert not misses, f"{name} on a side stream: {misses}"


def test_negative_control_a_call_on_a_stream_that_does_not_wait_misses(states, delay):
    """csr_sum with its inputs written on s behind the delay and the call on a second stream that does not wait for s: what a step
    on the wrong stream does.  It reads the decoy (all buffers are valid: nothing can fault) and must NOT give the expected bits.
    Over SIDE_STREAMS consecutive pairs of streams: a pair that shares a hardware queue is ordered by accident and gives the expected
    bits after all, which at most one pair in four may do."""
    st = states("csr_sum")
    want, decoy = _run(st, 0), _run(st, 1)
    seen = 0
    for i in range(SIDE_STREAMS):
        got, pending, ms = _behind_the_delay(st, delay, call_stream=torch.cuda.Stream(DEV))
        assert pending, "inconclusive: the delay had run out when the call returned"
        ordered = st.verdict(0, got, want) is None
        print(f"negative control, pair {i}: delay {delay.ms:.2f} ms, enqueue {ms:.3f} ms, {'ordered by accident' if ordered else 'missed'}")
        if not ordered:
            seen += 1
            assert st.verdict(1, got, decoy) is None, "the unordered call saw neither the real contents nor the decoy"
    assert seen >= SIDE_STREAMS - 1, f"only {seen} of {SIDE_STREAMS} calls that do not wait for their inputs' stream missed: the harness is blind"


# ---------------------------------------------------------------------------------------------------------------- b. no host round trip
class _SyncIsAnError:
    def __enter__(self):
        self.before = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode(self.before)


def test_the_sync_debug_mode_sees_a_host_read():
    x = torch.ones(1, device=DEV)
    torch.cuda.synchronize()
    with _SyncIsAnError():
        with pytest.raises(RuntimeError):
            x.item()
    assert torch.cuda.get_sync_debug_mode() == 0
    assert x.item() == 1.0


@pytest.mark.parametrize("name", contexts.NAMES)
def test_the_call_makes_no_host_round_trip(states, name):
    st = states(name)
    want = _run(st, 0)
    st.fill(0)
    st.poison()
    torch.cuda.synchronize()
    with _SyncIsAnError():
        outs = st.call()
    got = _snap(outs)
    torch.cuda.synchronize()
    miss = st.verdict(0, _host(got), want)
    assert miss is None, f"{name}: {miss}"


# ---------------------------------------------------------------------------------------------------------------- c. capture and replay
@pytest.mark.parametrize("name", contexts.NAMES)
def test_captured_and_replayed_on_new_contents(states, name):
    st = states(name)
    st.fill(0)
    st.poison()
    torch.cuda.synchronize()
    s = torch.cuda.Stream(DEV)                            # warm up on a side stream, as TwoHopEngine.capture does
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        st.call()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                         # one call: a linear graph on one stream
        outs = st.call()
    torch.cuda.synchronize()
    for v in (0, 1, 2):                                   # the real contents, the decoy, a third set with another n_dev
        st.fill(v)
        st.poison()
        graph.replay()
        got = _snap(outs)
        torch.cuda.synchronize()
        want = _run(st, v)
        miss = st.verdict(v, _host(got), want)
        assert miss is None, f"{name}: replay on contents {v}: {miss}"


# ---------------------------------------------------------------------------------------------------------------- d. second device
needs_two_gpus = pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs a second GPU: this machine has one")


@needs_two_gpus
@pytest.mark.parametrize("name", contexts.NAMES)
def test_on_the_second_device_the_bits_of_the_first(states, name):
    """Device 0 first, in this process: whatever the library configures once per process (the LDS reservations of the large
    kernels) is configured when device 1 runs."""
    st0 = states(name)
    want = _run(st0, 0)
    other = torch.device("cuda", 1)
    with torch.cuda.device(other):
        st1 = contexts.BY_NAME[name].build(other)
        st1.fill(0)
        st1.poison()
        got = _snap(st1.call())
        torch.cuda.synchronize(other)
        got = _host(got)
    assert torch.cuda.current_device() == 0
    miss = st1.verdict(0, got, want)
    assert miss is None, f"{name} on cuda:1: {miss}"


@needs_two_gpus
@pytest.mark.parametrize("name", contexts.NAMES)
def test_tensors_of_a_device_that_is_not_current_are_refused(states, name):
    other = torch.device("cuda", 1)
    with torch.cuda.device(other):
        st1 = contexts.BY_NAME[name].build(other)
        st1.fill(0)
        torch.cuda.synchronize(other)
    assert torch.cuda.current_device() == 0
    with pytest.raises(native.SageError, match=r"cuda:1 while cuda:0 is the current device"):
        st1.call()
    st0 = states(name)                                    # mixed: one input of a device-0 case moved to device 1
    st0.fill(0)
    key = next(iter(st0.inputs))
    t = st0.inputs[key]
    home = t.data
    try:
        t.data = home.to(other)
        with pytest.raises(native.SageError):
            st0.call()
    finally:
        t.data = home
    torch.cuda.synchronize()
    assert st0.verdict(0, _run(st0, 0), _run(st0, 0)) is None
