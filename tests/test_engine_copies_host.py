"""The two owners behind TwoHopEngine's private copies, engine._TableCopies and engine._WeightCopies, on CPU tensors: which copy
exists for which table, what a version move, a `.data` write and a forced sync do to it, and that every rewrite is in place.
The smallest shapes at which each rule can go wrong; no device, no library call."""
import pytest
import torch

from sage355.engine import _TableCopies, _WeightCopies

N = 5


def _table(d0, seed=0):
    return torch.randn(N, d0, generator=torch.Generator().manual_seed(seed))


def test_plain_table_is_read_in_place():
    src = _table(8)
    t = _TableCopies(src, 8, N)
    assert t.table is src and t.ld == 8 and t.node_order is None and t.new_of_old is None
    src[2] = 1.0
    t.sync()
    t.sync(force=True)
    assert t.table is src and t.version_key() == src._version


def test_padded_table_follows_the_version_counter_in_place():
    src = _table(6)
    t = _TableCopies(src, 6, N)
    assert t.table is not src and tuple(t.table.shape) == (N, 8) and t.ld == 8
    assert torch.equal(t.table[:, :6], src) and not t.table[:, 6:].any()
    ptr = t.table.data_ptr()
    src[2] = torch.arange(6.0)                           # moves the version counter
    t.sync()
    assert torch.equal(t.table[:, :6], src) and not t.table[:, 6:].any() and t.table.data_ptr() == ptr
    held = t.table.clone()
    src.data[3] = 7.0                                    # does not
    t.sync()
    assert torch.equal(t.table, held)
    t.sync(force=True)
    assert torch.equal(t.table[3, :6], torch.full((6,), 7.0)) and torch.equal(t.table[:, :6], src)
    assert not t.table[:, 6:].any() and t.table.data_ptr() == ptr


@pytest.mark.parametrize("form", ["ld9", "misaligned"])
def test_leading_dimension_and_alignment_get_a_private_copy(form):
    if form == "ld9":
        big = torch.randn(N, 9)
        src, ld = big[:, :8], 9
    else:
        flat = torch.randn(N * 8 + 4)
        off = 1 + (-flat.data_ptr() % 16) // 4              # one float past a 16-byte boundary
        src, ld = flat[off: off + N * 8].view(N, 8), 8
        assert src.data_ptr() % 16 == 4
    t = _TableCopies(src, ld, N)
    assert t.table is not src and t.ld % 4 == 0 and t.table.data_ptr() % 16 == 0 and t.table.stride(0) == t.ld
    assert torch.equal(t.table, src)


@pytest.mark.parametrize("d0", [8, 6])
def test_renumbering_by_degree(d0):
    src = _table(d0)
    t = _TableCopies(src, d0, N, degrees=torch.tensor([1, 3, 0, 3, 2]))
    assert t.node_order.tolist() == [1, 3, 4, 0, 2]                          # descending, stable
    assert t.new_of_old.dtype == torch.int32 and t.new_of_old[t.node_order].tolist() == list(range(N))
    assert t.table is not src and tuple(t.table.shape) == (N, 8) and t.ld == 8
    for i in range(N):
        assert torch.equal(t.table[i, :d0], src[t.node_order[i]])
    assert not t.table[:, d0:].any()
    ptr = t.table.data_ptr()
    src[3] = 9.0
    t.sync()
    assert torch.equal(t.table[1, :d0], torch.full((d0,), 9.0)) and torch.equal(t.table[:, :d0], src[t.node_order])
    assert not t.table[:, d0:].any() and t.table.data_ptr() == ptr


def test_slice_major_copy_is_built_once_and_refreshed_once_per_version(monkeypatch):
    monkeypatch.delenv("SAGE_TABLE_SLICED", raising=False)
    monkeypatch.delenv("SAGE_TABLE_SLICE_FLOATS", raising=False)
    src = _table(64)
    t = _TableCopies(src, 64, N)
    assert t.slice_floats == 32 and t.sliced is None                         # built at the first request
    sl = t.slice_major()
    assert tuple(sl.shape) == (2, N, 32)
    for s in range(2):
        for r in range(N):
            assert torch.equal(sl[s, r], src[r, 32 * s: 32 * s + 32])
    assert t.slice_major() is sl and t.sliced is sl                          # two requesters, one tensor
    ptr, stamp = sl.data_ptr(), t.sliced_version
    src[1] = 3.0
    assert t.slice_major() is sl and sl.data_ptr() == ptr and t.sliced_version == src._version != stamp
    assert torch.equal(sl[1, 1], torch.full((32,), 3.0))
    sl[0, 0, 0] = -123.0                                                     # a sentinel (through a view: the copy's own version moves,
    stamp = t.sliced_version                                                 # the table's does not): a second request copies nothing
    assert t.slice_major() is sl and float(sl[0, 0, 0]) == -123.0 and t.sliced_version == stamp
    src.data[4] = 5.0                                                        # unseen by the stamp ...
    assert not torch.equal(t.slice_major()[0, 4], src[4, :32])
    assert t.slice_major(force=True) is sl and torch.equal(sl[0, 4], src[4, :32]) and float(sl[0, 0, 0]) == float(src[0, 0])


def test_slice_major_copy_of_a_private_table_follows_the_callers_version(monkeypatch):
    monkeypatch.delenv("SAGE_TABLE_SLICED", raising=False)
    monkeypatch.delenv("SAGE_TABLE_SLICE_FLOATS", raising=False)
    src = _table(64)
    t = _TableCopies(src, 64, N, degrees=torch.tensor([1, 3, 0, 3, 2]))
    sl = t.slice_major()
    src[3] = 2.0                                                             # working row 1
    t.sync()
    assert t.slice_major() is sl and torch.equal(sl[:, 1].reshape(-1), torch.full((64,), 2.0))


@pytest.mark.parametrize("d0, kwargs", [(32, {}), (48, {}), (64, dict(concat=True)), (64, dict(slice_major=False))])
def test_slice_major_copy_refused_or_not_wanted(monkeypatch, d0, kwargs):
    """W = 32: 32 columns are one slice (two are needed), 48 are not whole slices; the concat encoder and slice_major=False want none."""
    monkeypatch.delenv("SAGE_TABLE_SLICED", raising=False)
    monkeypatch.delenv("SAGE_TABLE_SLICE_FLOATS", raising=False)
    t = _TableCopies(_table(d0), d0, N, **kwargs)
    assert t.slice_major() is None and t.slice_major(force=True) is None and t.sliced is None


def test_slice_width_and_switch_are_read_once_at_construction(monkeypatch):
    monkeypatch.setenv("SAGE_TABLE_SLICE_FLOATS", "64")
    monkeypatch.setenv("SAGE_TABLE_SLICED", "2")
    t = _TableCopies(_table(128), 128, N, concat=True)
    monkeypatch.setenv("SAGE_TABLE_SLICE_FLOATS", "32")
    monkeypatch.setenv("SAGE_TABLE_SLICED", "0")
    assert t.slice_floats == 64 and tuple(t.slice_major().shape) == (2, N, 64)
    assert _TableCopies(_table(128), 128, N).slice_major() is None          # SAGE_TABLE_SLICED=0: never


def test_padded_weights_follow_key_and_epoch_in_place():
    h1, d0, h2 = 30, 6, 5
    gen = torch.Generator().manual_seed(1)
    w1, w2 = torch.randn(h1, 2 * d0, generator=gen), torch.randn(h2, 2 * h1, generator=gen)
    wc = _WeightCopies(w1, w2, d0, concat=True)
    assert wc.padded and (wc.d0p, wc.h1p) == (8, 32)

    def check():
        w1p, w2p = wc.tensors()
        assert tuple(w1p.shape) == (32, 16) and tuple(w2p.shape) == (5, 64)
        keep1, keep2 = torch.zeros(32, 16, dtype=torch.bool), torch.zeros(5, 64, dtype=torch.bool)
        for c in range(2):
            assert torch.equal(w1p[:h1, c * 8: c * 8 + d0], w1[:, c * d0: (c + 1) * d0])
            assert torch.equal(w2p[:, c * 32: c * 32 + h1], w2[:, c * h1: (c + 1) * h1])
            keep1[:h1, c * 8: c * 8 + d0] = True
            keep2[:, c * 32: c * 32 + h1] = True
        assert not w1p[~keep1].any() and not w2p[~keep2].any()
        return w1p, w2p

    w1p, w2p = check()
    ptrs, key = (w1p.data_ptr(), w2p.data_ptr()), wc.version_key()
    with torch.no_grad():
        w1.add_(1.0)                                     # moves the key
    assert wc.version_key() != key
    w1p, w2p = check()
    assert (w1p.data_ptr(), w2p.data_ptr()) == ptrs
    held, key = w1p.clone(), wc.version_key()
    w1.data.mul_(2.0)                                    # does not ...
    assert wc.version_key() == key and torch.equal(wc.tensors()[0], held)
    wc.invalidate()                                      # ... until the epoch moves
    assert wc.version_key() != key
    w1p, w2p = check()
    assert (w1p.data_ptr(), w2p.data_ptr()) == ptrs and not torch.equal(w1p, held)


def test_unpadded_weights_are_the_callers_tensors():
    w1, w2 = torch.randn(32, 8), torch.randn(5, 32)
    wc = _WeightCopies(w1, w2, 8)
    assert not wc.padded and wc.tensors()[0] is w1 and wc.tensors()[1] is w2
