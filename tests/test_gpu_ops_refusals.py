"""Every tensor-taking wrapper of sage355.ops refuses a host tensor, a tensor of another dtype and (2-d fp32) a view whose inner stride
is not 1, in Python, before any library entry is called.  One table row per wrapper: a valid call at the smallest meaningful shape
(a graph of 3 nodes and 4 entries, one of them a self entry; dim 4; k = 2; 3 seed rows with one repeat; an embedding of 2 rows for the
indexed forms -- layer1_fused, whose smallest supported shape is dim 64 -> 32, apart).  The valid call runs once for real (shape and
finiteness only: other tests own the values); then native.lib is replaced by a stub that answers the host-arithmetic queries from the real
library and records every other entry, and each tensor argument is replaced in turn.  Nothing is launched after the valid calls.
Not in the table: csr_transpose, csr_transpose_grouped, group_rows, slice_major and as_ids, which are torch operations on the
tensors' own device (host tensors are valid there) and call no library entry."""
import collections
import ctypes

import pytest
import torch

from sage355 import native, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
WS_BYTES = 1 << 20                                        # more than any call here asks for (the largest, embed_grad_rows: 69120)
WRONG = {torch.int32: torch.int64, torch.int64: torch.int32, torch.float32: torch.float64, torch.uint8: torch.float32}
Case = collections.namedtuple("Case", "fn kwargs shape workspace wrong")


def _i32(*v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _f32(rows, cols, seed):
    return torch.randn(rows, cols, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _cases():
    """name -> Case.  kwargs: every argument of the valid call by name; shape: of the (first) tensor it returns; workspace: does the
    wrapper take workspace=; wrong: dtypes to use instead of WRONG's for the named arguments."""
    rowptr, col = torch.tensor([0, 2, 3, 4], dtype=torch.int64, device=DEV), _i32(0, 1, 2, 0)       # node 0 lists itself
    nodes, index = _i32(0, 2, 0), _i32(0, 1, 0)
    nbr, cnt, ids = _i32([0, 1], [1, 0], [2, 2]), _i32(2, 1, 2), _i32(0, 1, 2)                      # no empty set: no NaN rule in play
    one, flag = _i32(3), _i32(1)
    table, embed, grad = _f32(3, 4, 0), _f32(2, 4, 1), _f32(3, 4, 2)
    w, w_self = _f32(4, 4, 3), _f32(4, 8, 4)
    rowptr_t, col_t = ops.csr_transpose(rowptr, col)
    grouped = ops.csr_transpose_grouped(rowptr, col, index, 2, self_loop=True)
    rowptr_g, col_g = ops.group_rows(index, 2)
    h = ops.linear_act(table, w_self, self_tab=table)
    zeros = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=DEV)
    touched = lambda: (zeros(2, dtype=torch.int32), zeros(1, dtype=torch.int32), zeros(2, 4))
    sample = dict(rowptr=rowptr, col=col, nodes=nodes, k=2, seed=7, n_dev=one, any_nonempty=flag.clone(), out_nbr=zeros(3, 2, dtype=torch.int32),
                  out_cnt=zeros(3, dtype=torch.int32))
    seeds = dict(rowptr=rowptr, col=col, nodes=nodes, grad_out=grad, index=index, num_rows=2, self_loop=True, max_edges=4,
                 total_terms=zeros(1, dtype=torch.int64))
    sets = dict(grad_agg=grad, nbr=_i32([0, 1], [1, 0], [1, 1]), cnt=cnt, embed_rows=2, n_dev=one, row_order=ids)
    t64, w64 = ops.slice_major(_f32(3, 64, 5)), _f32(32, 64, 6)                                      # layer1_fused: [2, 3, 32] slices, 64 -> 32
    frontier = ops.Frontier(3 * (2 + 1), DEV)                                                        # room for every id and every self id
    return {
        "sample_neighbors": Case(ops.sample_neighbors, sample, (3, 2), False, {}),
        "sample_neighbors_wide": Case(ops.sample_neighbors_wide, sample, (3, 2), False, {}),
        "sample_neighbors_any": Case(ops.sample_neighbors_any, sample, (3, 2), False, {}),
        "frontier_insert": Case(ops.frontier_insert, dict(nbr=nbr, cnt=cnt, frontier=frontier, self_nodes=ids, n_dev=one), (3, 2), False, {}),
        "gather_mean": Case(ops.gather_mean, dict(table=table, nbr=nbr, cnt=cnt, slot_rows=ids, self_row=ids, any_nonempty=flag, n_dev=one,
                                                  out=zeros(3, 4)), (3, 4), False, {}),
        "gather_mean_backward": Case(ops.gather_mean_backward, dict(grad_out=grad, nbr=nbr, cnt=cnt, table_rows=3, slot_rows=ids, self_row=ids,
                                                                    n_dev=one, out=zeros(3, 4)), (3, 4), False, {}),
        "linear_act": Case(ops.linear_act, dict(agg=table, weight=w_self, self_tab=table, self_index=ids, n_dev=one, out=zeros(3, 4)),
                           (3, 4), False, {}),
        "linear_act_backward": Case(ops.linear_act_backward, dict(agg=table, weight=w_self, act=ops.ACT_RELU, out=h, grad_out=grad, self_tab=table,
                                                                  self_index=ids, n_dev=one), (4, 8), True, {}),
        "layer_forward": Case(ops.layer_forward, dict(table=table, nbr=nbr, cnt=cnt, weight=w_self, concat=True, self_index=ids, slot_rows=ids,
                                                      self_row=ids, any_nonempty=flag, n_dev=one, out=zeros(3, 4)), (3, 4), False, {}),
        "prepare_weights": Case(ops.prepare_weights, dict(weight=w64), (native.lib().sage_prepared_weight_bytes(64, 32, 0),), False, {}),
        "layer1_fused": Case(ops.layer1_fused, dict(table_sliced=t64, nbr=nbr, cnt=cnt, weight=w64, self_row=ids, any_nonempty=flag, n_dev=one,
                                                    out=zeros(3, 32), prepared=ops.prepare_weights(w64)), (3, 32), False, {}),
        "csr_mean": Case(ops.csr_mean, dict(rowptr=rowptr, col=col, table=table, nodes=nodes, self_loop=True, any_nonempty=flag, out=zeros(3, 4)),
                         (3, 4), True, {"table": torch.float16}),
        "csr_mean(index=)": Case(ops.csr_mean, dict(rowptr=rowptr, col=col, table=embed, nodes=nodes, any_nonempty=flag, index=index), (3, 4), True,
                                 {"table": torch.float16}),
        "csr_frontier": Case(ops.csr_frontier, dict(rowptr=rowptr, col=col, seeds=nodes, frontier=ops.CsrFrontier(3, DEV)), None, False, {}),
        "csr_mean_backward": Case(ops.csr_mean_backward, dict(rowptr=rowptr, col=col, rowptr_t=rowptr_t, col_t=col_t, grad_out=grad, nodes=nodes,
                                                              self_loop=True, out=zeros(3, 4)), (3, 4), True, {}),
        "csr_mean_backward_grouped": Case(ops.csr_mean_backward_grouped, dict(rowptr=rowptr, col=col, grouped=grouped, grad_out=grad,
                                                                              out=zeros(2, 4)), (2, 4), True, {}),
        "csr_mean_backward_rows": Case(ops.csr_mean_backward_rows, dict(seeds, out=zeros(2, 4)), (2, 4), True, {}),
        "csr_mean_backward_touched": Case(ops.csr_mean_backward_touched, dict(seeds, table=embed.clone(), lr=0.5, out=touched()), (2,), True, {}),
        "csr_sum": Case(ops.csr_sum, dict(rowptr=rowptr_g, col=col_g, table=table, out=zeros(2, 4)), (2, 4), True, {}),
        "row_order": Case(ops.row_order, dict(nodes=nodes, n_dev=one, out=zeros(3, dtype=torch.int32)), (3,), True, {}),
        "embed_grad": Case(ops.embed_grad, dict(sets, out=zeros(2, 4)), (2, 4), True, {}),
        "embed_grad_rows": Case(ops.embed_grad_rows, dict(sets, embed=embed.clone(), lr=0.5, out=touched()), (2,), True, {}),
        "xent_head": Case(ops.xent_head, dict(emb=table, w_cls=embed, labels=torch.tensor([0, 1, 1], device=DEV)), (1,), True, {}),
    }


NAMES = ["sample_neighbors", "sample_neighbors_wide", "sample_neighbors_any", "frontier_insert", "gather_mean", "gather_mean_backward",
         "linear_act", "linear_act_backward", "layer_forward", "prepare_weights", "layer1_fused", "csr_mean", "csr_mean(index=)", "csr_frontier",
         "csr_mean_backward", "csr_mean_backward_grouped", "csr_mean_backward_rows", "csr_mean_backward_touched", "csr_sum", "row_order",
         "embed_grad", "embed_grad_rows", "xent_head"]


@pytest.fixture(scope="module")
def cases():
    made = _cases()
    assert list(made) == NAMES
    return made


def _tensors(value):
    """The tensors a wrapper returned, in order: a tensor, a tuple or a dict of them (None entries dropped), a CsrFrontier's node list."""
    if isinstance(value, ops.CsrFrontier):
        return [value.nodes, value.count]
    if isinstance(value, dict):
        value = tuple(value.values())
    return [t for t in (value if isinstance(value, tuple) else (value,)) if isinstance(t, torch.Tensor)]


def _slots(kwargs):
    """(key, position or None) of every tensor among the arguments: a tensor, or an entry of a tuple (out=, grouped=)."""
    for key, v in kwargs.items():
        if isinstance(v, torch.Tensor):
            yield key, None
        elif isinstance(v, tuple):
            yield from ((key, i) for i, t in enumerate(v) if isinstance(t, torch.Tensor))


def _with(kwargs, key, pos, tensor):
    v = kwargs[key]
    if pos is not None:
        entries = list(v)
        entries[pos] = tensor
        tensor = type(v)(*entries) if hasattr(v, "_fields") else tuple(entries)
    return dict(kwargs, **{key: tensor})


def _bad_forms(t, wrong):
    """What must be refused in the place of a valid tensor t."""
    yield "a host copy", t.cpu()
    yield "dtype", t.to(wrong or WRONG[t.dtype])
    if t.dim() == 2 and t.dtype == torch.float32:
        yield "inner stride 2", t.repeat_interleave(2, dim=1)[:, ::2]


class _Stub:
    """Stands in for the loaded library: host arithmetic is the real library's, every other entry is recorded and launches nothing."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        if name.endswith(("_workspace_bytes", "_supported")) or name in ("sage_prepared_weight_bytes", "sage_last_error"):
            return getattr(self.real, name)

        def entry(*args):
            self.calls.append((name, args))
            return 0
        return entry


@pytest.fixture
def stub(monkeypatch):
    s = _Stub(native.lib())
    monkeypatch.setattr(native, "lib", lambda: s)
    return s


@pytest.mark.parametrize("name", NAMES)
def test_the_valid_call_runs(cases, name):
    case = cases[name]
    got = _tensors(case.fn(**case.kwargs))
    torch.cuda.synchronize()
    assert got and (case.shape is None or tuple(got[0].shape) == case.shape), [tuple(t.shape) for t in got]
    for t in got:
        assert not t.is_floating_point() or bool(torch.isfinite(t).all())


@pytest.mark.parametrize("name", NAMES)
def test_every_tensor_argument_is_checked_before_any_library_call(cases, stub, name):
    case = cases[name]
    slots = list(_slots(case.kwargs))
    assert slots
    for key, pos in slots:
        t = case.kwargs[key] if pos is None else case.kwargs[key][pos]
        for what, bad in _bad_forms(t, case.wrong.get(key)):
            where = f"{name}: {key}{'' if pos is None else [pos]} as {what}"
            try:
                case.fn(**_with(case.kwargs, key, pos, bad))
            except native.SageError:
                assert stub.calls == [], f"{where} was refused after {stub.calls[0][0]} had been called"
            else:
                pytest.fail(f"{where} was accepted")


@pytest.mark.parametrize("name", [n for n in NAMES if n not in ("sample_neighbors", "sample_neighbors_wide", "sample_neighbors_any",
                                                                 "frontier_insert", "gather_mean", "gather_mean_backward", "linear_act",
                                                                 "layer_forward", "prepare_weights", "layer1_fused", "csr_frontier")])
def test_a_workspace_is_a_uint8_tensor_on_the_device(cases, stub, name):
    case = cases[name]
    assert case.workspace
    for bad in (torch.zeros(WS_BYTES, dtype=torch.uint8), torch.zeros(WS_BYTES, device=DEV)):
        with pytest.raises(native.SageError):
            case.fn(**dict(case.kwargs, workspace=bad))
        assert stub.calls == []
    short = torch.zeros(16, dtype=torch.uint8, device=DEV)
    if name == "xent_head":                              # the stricter rule: a given workspace must be large enough
        with pytest.raises(native.SageError):
            case.fn(**dict(case.kwargs, workspace=short))
        assert stub.calls == []
        return
    case.fn(**dict(case.kwargs, workspace=short))        # a short one (a trainer's shared buffer) is replaced by a fresh one
    (entry, args), = stub.calls
    pointers = [a.value for a in args if isinstance(a, ctypes.c_void_p)]
    assert short.data_ptr() not in pointers, f"{entry} was handed the short workspace"
    given = torch.zeros(WS_BYTES, dtype=torch.uint8, device=DEV)
    stub.calls.clear()
    case.fn(**dict(case.kwargs, workspace=given))
    assert given.data_ptr() in [a.value for a in stub.calls[0][1] if isinstance(a, ctypes.c_void_p)], "a large enough workspace is used"


def test_the_workspace_cases_are_the_wrappers_that_take_one(cases):
    import inspect
    for name, case in cases.items():
        assert case.workspace == ("workspace" in inspect.signature(case.fn).parameters), name


def test_linear_act_backward_checks_its_shapes(cases, stub):
    case = cases["linear_act_backward"]
    kw = case.kwargs
    for bad in (dict(grad_out=kw["grad_out"][:2]),                                   # fewer rows than agg
                dict(weight=kw["weight"][:, :4].contiguous()),                        # not [self | agg] wide
                dict(weight=torch.zeros(4, 12, device=DEV)),
                dict(self_tab=torch.zeros(3, 8, device=DEV)),                         # another width than agg
                dict(out=kw["out"][:, :3].contiguous())):                             # fewer columns than the weight has rows
        with pytest.raises(native.SageError):
            case.fn(**dict(kw, **bad))
        assert stub.calls == []
