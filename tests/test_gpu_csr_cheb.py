"""The Chebyshev step sage_csr_cheb_step on the GPU: the bits of csr_sum at every group width, column block and load path, the full
step element-wise against fp64, the in-place form, a row's independence of its place, and a plan reused.

Bound of the full step (u = 2^-24, len_i entries in row i), derived and not tuned:
    |out - ref| <= u * (len_i + 4) * (|a| * sum_e |y[col e]| + |b| |y_i| + |g| |x_i|)      per element
        out = fma(a, S, fma(b, y_i, g * x_i)).  S is a sum of len_i terms in any grouping: len_i - 1 roundings of at most u times
        the sum of magnitudes each.  One product (g * x_i) and two fmas: one rounding each, of a quantity that the bracket bounds.
        a, b and g arrive as floats: u / 2 relative each, at most one more u on every term.  That is (len_i - 1) + 3 + 1 <=
        len_i + 4 units of u times the bracket; second-order terms are below u * (len_i + 4)^2 / 2 of a unit (2e-4 at 3000
        entries) and the reference is fp64.
    An empty row without b and g has bracket 0: the element is exactly +0."""
import functools

import numpy as np
import pytest
import torch

from sage355 import native, ops
from util import csr_row_sums

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
EDGE_LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1024, 1025, 3000]
NS = (1, 63, 65, 513, 1027)
DIMS = (1, 3, 4, 5, 60, 64, 68, 100, 124, 128, 132, 256, 260)


@functools.lru_cache(maxsize=None)
def edge_graph(n, seed):
    """N nodes whose rows have the EDGE_LENGTHS (as many of them as there are rows, from a seeded offset on) and 0..20 entries
    elsewhere; entries are random ids, so a row names some node twice (the kernel sums stored entries) -- rows 1, 5 and every
    7th repeat their first id on purpose --, rows 0, 3 and every 11th start with a self loop."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 21, n)
    where = rng.permutation(n)[:len(EDGE_LENGTHS)]
    lens[where] = np.roll(EDGE_LENGTHS, seed)[:len(where)]
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=rowptr[1:])
    col = rng.integers(0, n, int(rowptr[-1])).astype(np.int32)
    for r in range(n):
        if lens[r] > 0 and (r in (0, 3) or r % 11 == 0):
            col[rowptr[r]] = r
        if lens[r] > 1 and (r in (1, 5) or r % 7 == 0):
            col[rowptr[r] + 1] = col[rowptr[r]]
    return rowptr, col


def dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def block(n, dim, seed, pad=0):
    """A random fp32 [n, dim] device block, as a view of an [n, dim + pad] allocation filled with NaN outside the view."""
    rng = np.random.default_rng(seed)
    full = torch.full((n, dim + pad), float("nan"), device="cuda")
    view = full[:, :dim]
    view.copy_(torch.from_numpy((rng.standard_normal((n, dim)) * 10.0 ** rng.uniform(-2, 1, (n, 1))).astype(np.float32)))
    return view


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("dim", DIMS)
def test_plain_product_has_the_bits_of_csr_sum(dim):
    """a = 1, b = g = 0: out = fma(1, S, 0 * y) = S -- bit for bit csr_sum's row sums -- on both sides of each group width (16 lanes
    to dim 64, 32 to 128, 64 above on the float4 path; 16 / 32 columns on the scalar path), of the 256-column block, with 16-byte
    accesses and without (dim, or a leading dimension, no multiple of 4)."""
    for n in NS:
        rowptr, col = dev(*edge_graph(n, n % 7))
        if n >= 63:
            assert set(EDGE_LENGTHS) <= set(np.diff(edge_graph(n, n % 7)[0]).tolist())
        plan = ops.csr_cheb_plan(rowptr, col, dim)
        for pad in (0, 4, 3):
            y = block(n, dim, 100 * n + dim, pad)
            want = ops.csr_sum(rowptr, col, y)
            out = block(n, dim, 1, pad)
            got = ops.csr_cheb_step(plan, y, out=out)
            assert got.data_ptr() == out.data_ptr()
            assert torch.equal(bits(got), bits(want)), (n, dim, pad)
            if pad:
                assert bool(torch.isnan(out._base[:, dim:]).all()), "the step wrote outside its columns"
        assert torch.equal(bits(ops.csr_cheb_step(plan, y.contiguous(), a=1.0, b=0.0, g=0.0)), bits(want))


@pytest.mark.parametrize("n,dim,pad,with_x", [(65, 5, 0, True), (513, 100, 0, True), (513, 64, 4, False), (1027, 132, 0, True),
                                             (1027, 260, 3, True), (1027, 256, 0, False), (1, 4, 0, True)])
def test_full_step_against_fp64(n, dim, pad, with_x):
    rowptr_h, col_h = edge_graph(n, 3)
    rowptr, col = dev(rowptr_h, col_h)
    y = block(n, dim, 7 * n + dim, pad)
    x = block(n, dim, 11 * n + dim, pad) if with_x else None
    a, b, g = 0.0371, -1.2345678, 0.777 if with_x else 0.0
    got = ops.csr_cheb_step(ops.csr_cheb_plan(rowptr, col, dim), y, x=x, a=a, b=b, g=g).cpu().numpy().astype(np.float64)
    y64 = y.cpu().numpy().astype(np.float64)
    x64 = x.cpu().numpy().astype(np.float64) if with_x else np.zeros_like(y64)
    s, mass = csr_row_sums(rowptr_h, col_h, y64)
    ref = a * s + b * y64 + g * x64
    lens = np.diff(rowptr_h)[:, None]
    bound = U * (lens + 4) * (abs(a) * mass + abs(b) * np.abs(y64) + abs(g) * np.abs(x64))
    err = np.abs(got - ref)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print(f"N={n} dim={dim} pad={pad} x={with_x}: max |out - ref| / bound = {ratio:.3f}")
    assert np.all(err <= bound), (int(np.argmax(err / np.maximum(bound, 1e-300))), ratio)


@pytest.mark.parametrize("dim", [5, 60, 100, 260])
def test_out_is_x_gives_the_bits_of_a_separate_out(dim):
    n = 513
    rowptr, col = dev(*edge_graph(n, 2))
    plan = ops.csr_cheb_plan(rowptr, col, dim)
    y, x = block(n, dim, 1), block(n, dim, 2)
    want = ops.csr_cheb_step(plan, y, x=x, a=0.5, b=-0.25, g=-0.75)
    x_before = x.clone()
    got = ops.csr_cheb_step(plan, y, x=x, a=0.5, b=-0.25, g=-0.75, out=x)
    assert got.data_ptr() == x.data_ptr()
    assert torch.equal(bits(got), bits(want)) and not torch.equal(bits(x_before), bits(want))


@pytest.mark.parametrize("dim", [3, 60, 100, 256])
def test_a_row_has_the_bits_it_has_in_any_other_graph(dim):
    """S_i depends on row i's stored entries and y alone: the rows keep their bits when the graph's row order is rotated (another
    group, another wave, another block, other rows beside them), y staying indexed by id.  b = g = 0, so that no row reads its own y."""
    n, shift = 1027, 389
    rowptr_h, col_h = edge_graph(n, 5)
    lens = np.diff(rowptr_h)
    y = block(n, dim, 9)
    a = ops.csr_cheb_step(ops.csr_cheb_plan(*dev(rowptr_h, col_h), dim), y, a=1.5)
    order = np.roll(np.arange(n), shift)                              # new row j is old row order[j]
    rowptr_r = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens[order], out=rowptr_r[1:])
    col_r = np.concatenate([col_h[rowptr_h[r]:rowptr_h[r + 1]] for r in order]).astype(np.int32)
    b = ops.csr_cheb_step(ops.csr_cheb_plan(*dev(rowptr_r, col_r), dim), y, a=1.5)
    assert torch.equal(bits(a[torch.from_numpy(order).cuda()]), bits(b))


def test_one_plan_serves_three_steps():
    n, dim = 1027, 100
    rowptr, col = dev(*edge_graph(n, 4))
    plan = ops.csr_cheb_plan(rowptr, col, dim)
    assert plan.workspace.numel() == ops.csr_cheb_workspace_bytes(n, int(rowptr[-1]), dim)
    y = block(n, dim, 21)
    for t in range(3):                                                # the steps write the long rows' partials into the plan's workspace
        want = ops.csr_sum(rowptr, col, y)
        got = ops.csr_cheb_step(plan, y)
        assert torch.equal(bits(got), bits(want)), t
        y = got / got.abs().amax().clamp_min(1.0)


def test_wrapper_refusals():
    n, dim = 65, 8
    rowptr, col = dev(*edge_graph(n, 1))
    plan = ops.csr_cheb_plan(rowptr, col, dim)
    y = block(n, dim, 1)
    with pytest.raises(native.SageError, match="overlaps y"):
        ops.csr_cheb_step(plan, y, out=y)
    with pytest.raises(native.SageError, match="expected"):
        ops.csr_cheb_step(plan, block(n, dim + 4, 1))
    with pytest.raises(native.SageError, match="expected"):
        ops.csr_cheb_step(plan, y, x=block(n - 1, dim, 1))
    with pytest.raises(native.SageError):
        ops.csr_cheb_step(plan, y.cpu())
    with pytest.raises(native.SageError):
        ops.csr_cheb_step(plan, y.double())
