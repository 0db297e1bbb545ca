"""CPU check of native.ptr, the one way a tensor becomes a pointer of a library call: None is NULL, host memory is refused, and so
is memory of a GPU that is not the current device."""
import pytest
import torch

from sage355 import native


def test_ptr_passes_none_through_and_refuses_a_host_tensor():
    assert native.ptr(None) is None
    with pytest.raises(native.SageError, match="not on a GPU"):
        native.ptr(torch.zeros(1))


class _DeviceTensorStub:
    """What native.ptr looks at of a device tensor, without a GPU; data_ptr records that it was asked."""
    is_cuda = True
    shape = (3,)
    dtype = torch.float32

    def __init__(self, index):
        self.device = torch.device("cuda", index)
        self.asked = 0

    def data_ptr(self):
        self.asked += 1
        return 0x1000


def test_ptr_refuses_a_tensor_of_another_device_before_it_takes_its_address(monkeypatch):
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    other = _DeviceTensorStub(1)
    with pytest.raises(native.SageError, match=r"cuda:1.*cuda:0"):
        native.ptr(other)
    assert other.asked == 0
    with pytest.raises(native.SageError, match=r"cuda:1.*cuda:0"):
        native.on_current_device(other)
    own = _DeviceTensorStub(0)
    assert native.ptr(own).value == 0x1000 and own.asked == 1


def test_a_frontier_struct_is_checked_at_every_call_and_needs_only_keys_and_c(monkeypatch):
    """The wrappers take any object with a `keys` tensor and the struct `c` (tests build short frontiers of their own that way)."""
    import types

    from sage355 import ops
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    marker = object()
    assert ops._frontier_struct(types.SimpleNamespace(keys=_DeviceTensorStub(0), c=marker)) is marker
    with pytest.raises(native.SageError, match=r"cuda:1.*cuda:0"):
        ops._frontier_struct(types.SimpleNamespace(keys=_DeviceTensorStub(1), c=marker))


def test_ptr_follows_the_current_device(monkeypatch):
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 1)
    assert native.ptr(_DeviceTensorStub(1)).value == 0x1000
    zero = _DeviceTensorStub(0)
    with pytest.raises(native.SageError, match=r"cuda:0.*cuda:1"):
        native.ptr(zero)
    assert zero.asked == 0
