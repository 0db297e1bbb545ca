"""CPU checks of the classifier head's boundary (ABI 9, sage_xent_head: model.py:59-69 + model.py:249): the three symbols exist in the
header, the binding and the library; the size queries are host arithmetic; invalid calls are refused on the host before anything is
launched (so they are safe without a GPU); EngineTrainer takes the choice of head."""
import ctypes
import inspect
import os
import re

from sage355 import native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["sage_xent_head", "sage_xent_head_supported", "sage_xent_head_workspace_bytes"]


def _lib():
    if not os.path.exists(native.LIB_PATH):
        native.build()
    return native.lib()


def test_abi_is_9_and_header_binding_and_library_agree_on_the_head():
    L = _lib()
    assert native.ABI_VERSION == 9 and L.sage_abi_version() == 9
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "sage355.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(sage_[a-z0-9_]+)\s*\(", text))
    for name in NAMES:
        assert name in declared, f"{name} not declared in include/sage355.h"
        assert name in native.SYMBOLS, f"{name} missing from native.SYMBOLS"
        assert hasattr(L, name), f"{name} not exported by the library"
    for macro, value in (("SAGE_HEAD_MAX_CLASSES", native.HEAD_MAX_CLASSES), ("SAGE_HEAD_MAX_DIM", native.HEAD_MAX_DIM),
                         ("SAGE_HEAD_RANGE_ROWS", native.HEAD_RANGE_ROWS)):
        assert re.search(rf"#define\s+{macro}\s+{value}\b", text), f"{macro} != {value} in the header"
    assert (native.HEAD_MAX_CLASSES, native.HEAD_MAX_DIM, native.HEAD_RANGE_ROWS) == (64, 256, 64)


def test_supported_shapes_and_workspace_size_are_host_arithmetic():
    L = _lib()
    for dim, c in ((128, 7), (4, 1), (256, 64)):
        assert L.sage_xent_head_supported(dim, c) == 1, (dim, c)
    for dim, c in ((130, 7), (260, 7), (128, 65), (128, 0)):
        assert L.sage_xent_head_supported(dim, c) == 0, (dim, c)
        assert L.sage_xent_head_workspace_bytes(4096, dim, c) == 0, (dim, c)
    tiles = 4096 // native.HEAD_RANGE_ROWS
    assert tiles == 64
    assert L.sage_xent_head_workspace_bytes(4096, 128, 16) >= tiles * 16 * 128 * 4
    assert L.sage_xent_head_workspace_bytes(1, 4, 1) >= 4 * 4 + 4
    assert L.sage_xent_head_workspace_bytes(0, 128, 16) == 0


def _call(L, emb, w, labels, n, scores, pred, loss, gemb, gw, ws, ws_bytes, dim=128, c=7, lde=128, ldw=128, lds=7, ldg=128, ldgw=128):
    return L.sage_xent_head(emb, lde, dim, w, ldw, c, labels, n, ctypes.c_float(1.0 / max(n, 1)), scores, lds, pred, loss, gemb, ldg, gw, ldgw,
                            ws, ws_bytes, None)


def test_invalid_calls_are_refused_on_the_host_before_any_launch():
    """None of these calls launches anything: the addresses below are never dereferenced on the host and never reach a kernel."""
    L = _lib()
    assert _call(L, None, None, None, 8, None, None, None, None, None, None, 0) == native.EINVAL
    assert b"NULL" in L.sage_last_error()
    A = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(9)]              # 16-byte aligned stand-ins for device arrays
    emb, w, labels, scores, pred, loss, gemb, gw, ws = A
    big = 1 << 30
    # gradients / loss without labels
    assert _call(L, emb, w, None, 8, None, None, None, gemb, gw, ws, big) == native.EINVAL
    assert b"labels" in L.sage_last_error()
    assert _call(L, emb, w, None, 8, scores, pred, loss, None, None, ws, big) == native.EINVAL
    # no rows; leading dimensions shorter than the widths
    assert _call(L, emb, w, labels, 0, scores, pred, loss, gemb, gw, ws, big) == native.EINVAL
    assert _call(L, emb, w, labels, 8, scores, pred, loss, gemb, gw, ws, big, lde=124) == native.EINVAL
    assert _call(L, emb, w, labels, 8, scores, pred, loss, gemb, gw, ws, big, lds=6) == native.EINVAL
    assert _call(L, emb, w, labels, 8, scores, pred, loss, gemb, gw, ws, big, ldgw=64) == native.EINVAL
    # shapes, strides and alignments the kernel does not take
    assert _call(L, emb, w, labels, 8, scores, pred, loss, gemb, gw, ws, big, dim=130, lde=132, ldw=132, ldg=132, ldgw=132) == native.EUNSUPPORTED
    assert _call(L, emb, w, labels, 8, scores, pred, loss, gemb, gw, ws, big, dim=260, lde=260, ldw=260, ldg=260, ldgw=260) == native.EUNSUPPORTED
    assert _call(L, emb, w, labels, 8, scores, pred, loss, gemb, gw, ws, big, c=65, lds=65) == native.EUNSUPPORTED
    assert _call(L, emb, w, labels, 8, scores, pred, loss, gemb, gw, ws, big, c=0, lds=0) == native.EUNSUPPORTED
    assert _call(L, emb, w, labels, 8, scores, pred, loss, gemb, gw, ws, big, lde=130) == native.EUNSUPPORTED
    assert _call(L, ctypes.c_void_p(0x10004), w, labels, 8, scores, pred, loss, gemb, gw, ws, big) == native.EUNSUPPORTED
    # short workspace
    need = L.sage_xent_head_workspace_bytes(8, 128, 7)
    assert _call(L, emb, w, labels, 8, scores, pred, loss, gemb, gw, ws, need - 1) == native.ENOSPACE
    assert b"workspace" in L.sage_last_error()


def test_engine_trainer_takes_the_head_and_defaults_to_torch():
    from sage355.train import EngineTrainer, run_engine_training
    assert inspect.signature(EngineTrainer.__init__).parameters["head"].default == "torch"
    assert inspect.signature(run_engine_training).parameters["head"].default == "torch"
    assert callable(EngineTrainer.predict)
