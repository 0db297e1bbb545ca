"""CPU check of native.ptr, the one way a tensor becomes a pointer of a library call: None is NULL, host memory is refused."""
import pytest
import torch

from sage355 import native


def test_ptr_passes_none_through_and_refuses_a_host_tensor():
    assert native.ptr(None) is None
    with pytest.raises(native.SageError):
        native.ptr(torch.zeros(1))
