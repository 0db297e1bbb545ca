"""CPU checks of the full-neighbourhood mean's C ABI (sage_csr_mean): argument validation before any launch, the workspace
query, and that the whole-graph inference module imports without a GPU."""
import importlib

from sage355 import native


def test_csr_mean_rejects_bad_arguments_before_any_launch():
    L = native.lib()
    # every array NULL: whatever else is wrong, nothing can be launched
    args = dict(num_nodes=10, n=5, max_edges=100, table_rows=10, ld=4, dim=4, self_loop=0, ldo=4)

    def call(**kw):
        a = dict(args, **kw)
        return L.sage_csr_mean(None, None, a["num_nodes"], None, a["n"], a["max_edges"], None, a["table_rows"], a["ld"], a["dim"],
                               a["self_loop"], None, None, a["ldo"], None, 0, None)

    assert call() == native.EINVAL and b"NULL" in L.sage_last_error()
    for kw, word in [(dict(dim=0), b"dim"), (dict(ld=3), b"ld"), (dict(ldo=2), b"ldo"), (dict(n=-1), b"n ="),
                     (dict(n=11), b"node list"), (dict(num_nodes=-1), b"num_nodes"), (dict(max_edges=-1), b"max_edges"),
                     (dict(table_rows=0), b"table_rows"), (dict(self_loop=2), b"self_loop")]:
        assert call(**kw) == native.EINVAL, kw
        assert word in L.sage_last_error(), (kw, L.sage_last_error())


def test_csr_mean_workspace_query():
    L = native.lib()
    ws = L.sage_csr_mean_workspace_bytes
    assert ws(-1, 10, 4) == 0 and ws(10, -1, 4) == 0 and ws(10, 10, 0) == 0
    prev = None
    for n in (0, 1, 100, 2048, 2049, 1 << 20):
        for e in (0, 511, 512, 513, 10_000, 30_000_000):
            for d in (1, 3, 50, 256):
                b = ws(n, e, d)
                assert b > 0 and b % 256 == 0, (n, e, d, b)
                assert ws(n + 1, e, d) >= b and ws(n, e + 1, d) >= b and ws(n, e, d + 1) >= b, (n, e, d)
    # the partial sums: one [dim] row per chunk of a row longer than the chunk (at most max_edges / chunk + long rows)
    assert native.CSR_MEAN_CHUNK == 512
    assert ws(1, 100 * 512, 256) - ws(1, 0, 256) >= 100 * 256 * 4


def test_inference_module_imports_without_gpu():
    mod = importlib.import_module("sage355.inference")
    for name in ("layer_all_nodes", "embed_all_nodes", "embed_all_from_modules"):
        assert callable(getattr(mod, name))
