"""CPU checks of the wide sampler's boundary (sage_sample_neighbors_wide: aggregators.py:42-48 for fanouts above SAGE_MAX_FANOUT, up to
SAGE_MAX_FANOUT_WIDE): the symbol exists in the header, the binding and the library; invalid calls are refused on the host before anything
is launched (so they are safe without a GPU); the Encoder routes the fanouts to the right path.

oracle/sampler_ref.c stops at k = 64, so the expected sets of the GPU tests (test_gpu_sample_wide.py, test_gpu_two_hop_wide.py) come from
`wide_ref` below: the rule of that file's header comment restated in Python for any k, with the oracle's Philox block function and the walk
of test_sampler_kat.py::py_sample.  Here it is checked against the C oracle at the fanouts both take."""
import ctypes
import os
import re

import numpy as np

from oracle import sampler_ref
from sage355 import native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32 = 0xFFFFFFFF


def wide_ref_row(rowptr, col, v, k, seed, tag):
    """The ids sampler_ref.c's rule gives node v (any k): the whole row when deg <= k, else Floyd's walk over Philox draws."""
    if not 0 <= v < len(rowptr) - 1:
        return []                                         # ids outside [0, num_nodes) are empty rows
    s, deg = int(rowptr[v]), int(rowptr[v + 1] - rowptr[v])
    if deg <= k:
        return [int(x) for x in col[s:s + deg]]
    key = (seed & M32, seed >> 32)
    pos, seen = [], set()
    for i in range(k):
        if i % 4 == 0:
            blk = sampler_ref.philox((v & M32, tag, i // 4, 0), key)
        j = deg - k + i
        t = (blk[i % 4] * (j + 1)) >> 32
        p = j if t in seen else t
        pos.append(p)
        seen.add(p)
    return [int(col[s + p]) for p in pos]


def wide_ref(rowptr, col, nodes, k, seed, tag):
    """-> (nbr int32 [n, k] padded with -1, cnt int32 [n]): what sage_sample_neighbors_wide must write."""
    nbr = np.full((len(nodes), k), -1, dtype=np.int32)
    cnt = np.zeros(len(nodes), dtype=np.int32)
    rows = {}
    for r, v in enumerate(nodes):
        v = int(v)
        if v not in rows:
            rows[v] = wide_ref_row(rowptr, col, v, k, seed, tag)
        cnt[r] = len(rows[v])
        nbr[r, :cnt[r]] = rows[v]
    return nbr, cnt


def _lib():
    if not os.path.exists(native.LIB_PATH):
        native.build()
    return native.lib()


def test_header_binding_and_library_agree_on_the_wide_sampler():
    L = _lib()
    assert native.ABI_VERSION == 9 and L.sage_abi_version() == 9          # additive: the ABI version does not move
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "sage355.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(sage_[a-z0-9_]+)\s*\(", text))
    name = "sage_sample_neighbors_wide"
    assert name in declared, f"{name} not declared in include/sage355.h"
    assert name in native.SYMBOLS, f"{name} missing from native.SYMBOLS"
    assert hasattr(L, name), f"{name} not exported by the library"
    assert L.sage_sample_neighbors_wide.argtypes == L.sage_sample_neighbors.argtypes
    assert re.search(rf"#define\s+SAGE_MAX_FANOUT_WIDE\s+{native.MAX_FANOUT_WIDE}\b", text)
    assert re.search(rf"#define\s+SAGE_MAX_FANOUT\s+{native.MAX_FANOUT}\b", text)
    assert (native.MAX_FANOUT, native.MAX_FANOUT_WIDE) == (64, 1024)


def _call(L, rowptr, col, nodes, nbr, cnt, n=8, k=100, num_nodes=1000, frontier=None, insert_self=0, nbr_slot=None, self_slot=None):
    return L.sage_sample_neighbors_wide(rowptr, col, num_nodes, nodes, n, None, k, 7, native.TAG_OUTER, nbr, cnt, None, frontier, insert_self,
                                        nbr_slot, self_slot, None)


def test_invalid_calls_are_refused_on_the_host_before_any_launch():
    """None of these calls launches anything: the addresses below are never dereferenced on the host and never reach a kernel."""
    L = _lib()
    A = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(11)]            # 16-byte aligned stand-ins for device arrays
    rowptr, col, nodes, nbr, cnt, keys, rows, fnodes, count, nbr_slot, self_slot = A
    assert _call(L, None, None, None, None, None) == native.EINVAL
    assert b"NULL" in L.sage_last_error()
    for missing in range(5):
        args = [rowptr, col, nodes, nbr, cnt]
        args[missing] = None
        assert _call(L, *args) == native.EINVAL and b"NULL" in L.sage_last_error()
    for k in (0, -1, native.MAX_FANOUT_WIDE + 1):
        assert _call(L, rowptr, col, nodes, nbr, cnt, k=k) == native.EINVAL
        assert b"k = " in L.sage_last_error() and b"1024" in L.sage_last_error()
    assert _call(L, rowptr, col, nodes, nbr, cnt, n=-1) == native.EINVAL
    assert _call(L, rowptr, col, nodes, nbr, cnt, num_nodes=0) == native.EINVAL
    assert _call(L, rowptr, col, nodes, nbr, cnt, num_nodes=1 << 31) == native.EINVAL
    assert b"num_nodes" in L.sage_last_error()
    # the frontier: capacity >= 2 n (k + insert_self), a power of two; its slot outputs must be there
    n, k = 8, 100

    def frontier(capacity):
        return native.Frontier(keys.value, rows.value, capacity, fnodes.value, count.value, 4096)

    assert _call(L, rowptr, col, nodes, nbr, cnt, n=n, k=k, frontier=frontier(1024), insert_self=1, nbr_slot=nbr_slot,
                 self_slot=self_slot) == native.EINVAL                     # 1024 < 2 * 8 * 101 = 1616
    assert b"capacity" in L.sage_last_error()
    assert _call(L, rowptr, col, nodes, nbr, cnt, n=n, k=k, frontier=frontier(2000), insert_self=1, nbr_slot=nbr_slot,
                 self_slot=self_slot) == native.EINVAL                     # large enough, not a power of two
    assert _call(L, rowptr, col, nodes, nbr, cnt, n=n, k=k, frontier=frontier(2048), insert_self=0) == native.EINVAL
    assert b"nbr_slot" in L.sage_last_error()
    assert _call(L, rowptr, col, nodes, nbr, cnt, n=n, k=k, frontier=frontier(2048), insert_self=1, nbr_slot=nbr_slot) == native.EINVAL
    assert b"self_slot" in L.sage_last_error()
    # n = 0 is a valid call that launches nothing
    assert _call(L, rowptr, col, nodes, nbr, cnt, n=0) == 0
    # the narrow entry keeps its limit
    assert L.sage_sample_neighbors(rowptr, col, 1000, nodes, 8, None, 65, 7, 1, nbr, cnt, None, None, 0, None, None, None) == native.EINVAL


def _random_csr(rng, n, max_deg):
    deg = rng.integers(0, max_deg, n)
    deg[rng.integers(0, n, 3)] = 4 * max_deg          # a few hubs
    rowptr = np.zeros(n + 1, np.int64)
    rowptr[1:] = np.cumsum(deg)
    col = np.concatenate([np.sort(rng.choice(10 * n, d, replace=False)) for d in deg] + [np.zeros(0, np.int64)]).astype(np.int32)
    return rowptr, col


def test_restatement_equals_the_c_oracle_where_both_apply():
    rng = np.random.default_rng(9)
    rowptr, col = _random_csr(rng, 300, 90)
    nodes = rng.permutation(300).astype(np.int32)
    for k in (1, 25, 64):
        for seed, tag in ((0xC0FFEE1234, native.TAG_INNER), (0xDEADBEEFCAFEF00D, native.TAG_OUTER)):
            want_nbr, want_cnt = sampler_ref.sample_neighbors(rowptr, col, nodes, k, seed, tag)
            nbr, cnt = wide_ref(rowptr, col, nodes, k, seed, tag)
            assert np.array_equal(cnt, want_cnt) and np.array_equal(nbr, want_nbr)
    # above the oracle's limit: still k distinct members of the row, the whole row when deg <= k
    nbr, cnt = wide_ref(rowptr, col, nodes, 100, 5, native.TAG_INNER)
    deg = np.diff(rowptr)[nodes]
    assert np.array_equal(cnt, np.minimum(deg, 100)) and (deg > 100).any()
    for r, v in enumerate(nodes):
        row = nbr[r, :cnt[r]].tolist()
        assert len(set(row)) == len(row) and set(row) <= set(col[rowptr[v]:rowptr[v + 1]].tolist())


def _stack(num_sample, gcn=True):
    """The model.py:214-222 wiring."""
    import torch.nn as nn
    from sage355.aggregators import MeanAggregator
    from sage355.encoders import Encoder
    adj = {i: {(i + 1) % 50, (i + 7) % 50} for i in range(50)}
    features = nn.Embedding(50, 8)
    features.weight.requires_grad = False
    agg1 = MeanAggregator(features, cuda=False)
    enc1 = Encoder(features, 8, 4, adj, agg1, num_sample=num_sample, gcn=gcn, cuda=False)
    agg2 = MeanAggregator(lambda nodes: enc1(nodes).t(), cuda=False)
    enc2 = Encoder(lambda nodes: enc1(nodes).t(), enc1.embed_dim, 4, adj, agg2, num_sample=num_sample, base_model=enc1, gcn=gcn, cuda=False)
    return enc1, enc2


def test_encoder_routes_fanouts_to_the_engine_the_operators_or_neither():
    for gcn in (True, False):
        enc1, enc2 = _stack(100, gcn)
        assert not enc2._can_fuse_two_hop() and enc2._can_two_hop_ops()
        assert not enc1._can_two_hop_ops()                 # a table Encoder is not a stack
        enc1, enc2 = _stack(10, gcn)
        assert enc2._can_fuse_two_hop() and not enc2._can_two_hop_ops()
        for num_sample in (2000, None):
            enc1, enc2 = _stack(num_sample, gcn)
            assert not enc2._can_fuse_two_hop() and not enc2._can_two_hop_ops()
    # one wide layer is enough, either of them; the limits are inclusive
    enc1, enc2 = _stack(10)
    enc2.num_sample = 65
    assert not enc2._can_fuse_two_hop() and enc2._can_two_hop_ops()
    enc1.num_sample, enc2.num_sample = 1024, 64
    assert not enc2._can_fuse_two_hop() and enc2._can_two_hop_ops()
    enc1.num_sample = 1025
    assert not enc2._can_two_hop_ops()
    enc1.num_sample, enc2.fuse_base_model = 100, False
    assert not enc2._can_two_hop_ops()


def test_every_wide_kernel_keeps_its_slots_in_registers(tmp_path):
    """A lane's slots live in a register array; an index the compiler cannot resolve would move it to scratch memory.  The compiler's
    resource report (the flags of csrc/Makefile plus the remark) must show zero scratch for all ten instantiations."""
    import subprocess
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    res = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(REPO, "include"), "-I" + native.CSRC_DIR,
                          "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(native.CSRC_DIR, "sage_sample_wide.hip"),
                          "-o", str(tmp_path / "sage_sample_wide.o")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    names = re.findall(r"Function Name: (\S*sample_wide_kernel\S*)", res.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", res.stderr)]
    assert len(set(names)) == 10 and len(scratch) == len(names), names
    assert all(x == 0 for x in scratch), list(zip(names, scratch))
