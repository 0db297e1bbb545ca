"""CPU checks of the operator-case registry (tests/contexts.py): it stays complete -- every entry point of the C ABI is claimed by a
case or excluded with a reason, so a new entry point that is in neither fails here -- and its contents are what the cases' shapes
promise (a row, a transposed row and a group past one 512-entry chunk; three sets of contents that really differ)."""
import inspect

import numpy as np
import torch

import contexts
from sage355 import native, ops


def test_every_entry_point_is_claimed_by_a_case_or_excluded_with_a_reason():
    claimed = contexts.claimed()
    unknown = sorted((set(claimed) | set(contexts.EXCLUDED)) - set(native.SYMBOLS))
    assert not unknown, f"not entry points of the library: {unknown}"
    both = sorted(set(claimed) & set(contexts.EXCLUDED))
    assert not both, f"claimed by a case and excluded: {both}"
    missing = [s for s in native.SYMBOLS if s not in claimed and s not in contexts.EXCLUDED]
    assert not missing, f"neither claimed by a case of tests/contexts.py nor in its exclusion table: {missing}"
    for table in (contexts.EXCLUDED, contexts.EXCLUDED_WRAPPERS):
        for name, reason in table.items():
            assert isinstance(reason, str) and len(reason) > 20, f"{name}: an exclusion needs its reason"


def test_every_launching_wrapper_of_ops_is_a_case_or_excluded():
    """The public functions of sage355.ops whose body calls a library entry that launches: each one's entries are claimed (so it is a
    case) or it is named in the exclusion tables."""
    claimed = contexts.claimed()
    for name, fn in inspect.getmembers(ops, inspect.isfunction):
        if name.startswith("_") or fn.__module__ != ops.__name__ or name in contexts.EXCLUDED_WRAPPERS:
            continue
        src = inspect.getsource(fn)
        used = [s for s in native.SYMBOLS if ("." + s + "(") in src]
        for s in used:
            assert s in claimed or s in contexts.EXCLUDED, f"ops.{name} calls {s}, which no case claims"


def test_the_case_names_are_unique_and_every_claim_names_its_operator():
    assert len(set(contexts.NAMES)) == len(contexts.NAMES) >= 25
    for c in contexts.CASES:
        assert c.claims, c.name


def test_the_graphs_take_the_multi_launch_paths_and_the_contents_differ():
    chunk = native.CSR_MEAN_CHUNK
    seen = []
    for v in contexts.VARIANTS:
        rowptr, col = contexts.graph_variant(v)
        deg = np.diff(rowptr)
        assert len(deg) == contexts.N == 65 and rowptr[0] == 0 and rowptr[-1] == contexts.E == len(col) and deg.min() >= 0
        assert deg[contexts.LONG[v]] > chunk and np.sum(deg > chunk) == 1 and col.min() >= 0 and col.max() < contexts.N
        rowptr_t, _ = ops.csr_transpose(torch.from_numpy(rowptr), torch.from_numpy(col))
        assert int((rowptr_t[1:] - rowptr_t[:-1])[contexts.HOT[v]]) > chunk
        g = ops.csr_transpose_grouped(torch.from_numpy(rowptr), torch.from_numpy(col), torch.from_numpy(contexts._index(v)), contexts.GROUPS)
        assert g.col.numel() == contexts.E and int((g.rowptr[1:] - g.rowptr[:-1]).max()) > chunk
        nbr, cnt, self_row = contexts.sets_variant(v)
        assert nbr.shape == (65, 9) and {0, 1, 9} <= set(cnt.tolist()) and nbr.min() >= 0 and nbr.max() < contexts.SETS_ROWS
        assert self_row.max() < contexts.SETS_ROWS and (self_row == -1).any()
        for must in (contexts.LONG[v], contexts.HOT[v]):
            nodes = contexts._nodes(v, must=must)
            assert must in nodes and len(set(nodes.tolist())) == len(nodes) == 50
        seen.append((rowptr, col, nbr, cnt))
    for a in range(3):
        for b in range(a + 1, 3):
            assert all(not np.array_equal(x, y) for x, y in zip(seen[a], seen[b]))
    assert len(set(contexts.N_DEV)) == 3 and max(contexts.N_DEV) == contexts.N and min(contexts.N_DEV) < contexts.N - 1


def test_state_fills_in_place_and_judges_by_bits():
    st = contexts.State("cpu")
    x = st.add("x", [np.full(4, float(v), dtype=np.float32) for v in contexts.VARIANTS])
    out = st.out(4)
    ws = st.workspace(8)
    where = x.data_ptr()
    for v in contexts.VARIANTS:
        st.fill(v)
        assert x.data_ptr() == where and bool((x == v).all())
    st.poison()
    assert bool((out == contexts.SENTINEL_F).all()) and bool((ws == contexts.STALE_BYTE).all())
    a = torch.tensor([0.0, float("nan")])
    assert st.verdict(0, [a], [a.clone()]) is None                       # bits, so a NaN equals itself
    assert st.verdict(0, [a], [torch.tensor([-0.0, float("nan")])]) is not None
    assert st.verdict(0, [a], [a, a]) is not None
