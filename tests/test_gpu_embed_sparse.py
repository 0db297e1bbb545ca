"""sage_embed_grad_rows on the GPU, the kernel alone: the touched rows of an embedding's gradient, bit for bit the rows sage_embed_grad
stores, at every run length at which the kernels take another path, with the 15 ids lying densely, spread over 2^17 rows and spread
over 2^31 - 1; the SGD update of those rows in place (one rounding) and of nothing else; the live-row count, the clamp, the layout
independence and the capacity rule."""
import numpy as np
import pytest
import torch

from sage355 import native, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [0, 1, 2, 63, 64, 65, 0, 511, 512, 513, 1024, 1025, 1537, 2600, 0]        # terms per embedding row: tests/test_gpu_embed_grad.py's
R, TERMS = len(SIZES), sum(SIZES)
FANOUTS = [1, 7, 64]
WIDTHS = [4, 52, 128, 132]
U = 2.0 ** -24
TOUCHED = np.nonzero(SIZES)[0]                                                     # the ids with a run, ascending
NU = len(TOUCHED)

_cases = {}


def case(k):
    """(nodes, nbr [n, k], cnt [n]) on the host: the multiset of keys (embedding row e SIZES[e] times), permuted and cut into rows of
    k slots.  Row fills cycle through k, k, 0, 1, k - 1 and k with cnt = k + 3 (cnt > k: the kernel takes k); padding is -1."""
    if k not in _cases:
        rng = np.random.default_rng(40 + k)
        keys = rng.permutation(np.repeat(np.arange(R), SIZES)).astype(np.int32)
        fills = [(k, k), (k, k), (0, 0), (min(1, k), min(1, k)), (k - 1, k - 1), (k, k + 3)]      # (terms held, cnt stored)
        rows, cnts, pos, i = [], [], 0, 0
        while pos < TERMS:
            held, stored = fills[i % len(fills)]
            i += 1
            held = min(held, TERMS - pos)
            if held < min(stored, k):
                stored = held
            row = np.full(k, -1, dtype=np.int32)
            row[:held] = keys[pos:pos + held]
            pos += held
            rows.append(row)
            cnts.append(stored)
        nbr, cnt = np.stack(rows), np.asarray(cnts, dtype=np.int32)
        n = len(cnt)
        assert {0, min(1, k), k - 1, k + 3} <= set(cnt.tolist()) and n >= 2 * 64
        nodes = rng.permutation(10 * n)[:n].astype(np.int32)                                     # distinct node ids, in no order
        held = np.minimum(cnt, k)
        assert np.array_equal(np.bincount(np.concatenate([nbr[t, :held[t]] for t in range(n)]), minlength=R), SIZES)
        _cases[k] = (nodes, nbr, cnt)
    return _cases[k]


PLACEMENTS = {"dense": R, "spread": 1 << 17, "huge": (1 << 31) - 1}


def id_map(placement):
    """The 15 ids mapped increasingly into [0, embed_rows): ids 0 and embed_rows - 1 are images (of the run-less ids 0 and 14), and the
    last id with a run, 13, lands on embed_rows - 2, the highest row that can hold a run beside them."""
    rows = PLACEMENTS[placement]
    if placement == "dense":
        return rows, np.arange(R, dtype=np.int64)
    m = np.arange(R, dtype=np.int64) * ((rows - 1) // (R + 1))
    m[R - 1], m[R - 2] = rows - 1, rows - 2
    assert m[0] == 0 and np.all(np.diff(m) > 0)
    return rows, m


def placed(k, placement):
    """(embed_rows, id map, nbr with the ids mapped; padding stays -1)."""
    rows, m = id_map(placement)
    nbr = case(k)[1]
    return rows, m, np.where(nbr >= 0, m[np.maximum(nbr, 0)], -1).astype(np.int32)


_grads, _refs, _dense = {}, {}, {}


def grad_of(k, dim):
    if (k, dim) not in _grads:
        n = case(k)[1].shape[0]
        _grads[(k, dim)] = torch.randn(n, dim, generator=torch.Generator().manual_seed(1000 * k + dim))
    return _grads[(k, dim)]


def reference(k, dim):
    """fp64 sums of grad_agg[t] / c_t per embedding row (ids 0..14), and the sums of the terms' magnitudes."""
    if (k, dim) not in _refs:
        _, nbr, cnt = case(k)
        g = grad_of(k, dim).double().numpy()
        ref, mag = np.zeros((R, dim)), np.zeros((R, dim))
        for t in range(nbr.shape[0]):
            c = min(int(cnt[t]), k)
            for j in range(c):
                e = int(nbr[t, j])
                ref[e] += g[t] / c
                mag[e] += np.abs(g[t]) / c
        _refs[(k, dim)] = (ref, mag)
    return _refs[(k, dim)]


def dense_rows(k, dim):
    """ops.embed_grad at embed_rows = 15, rows TOUCHED: the bits every placement has to give.  Computed once."""
    if (k, dim) not in _dense:
        _, nbr, cnt = case(k)
        nbr_d, cnt_d = dev(nbr, cnt)
        _dense[(k, dim)] = ops.embed_grad(grad_of(k, dim).to(DEV), nbr_d, cnt_d, R)[torch.from_numpy(TOUCHED).to(DEV)].clone()
    return _dense[(k, dim)]


def check(out, k, dim, what):
    """out [NU, dim], the touched rows: gamma_m * sum|terms|, m = min(c, 512) + ceil(c / 512) + 1 for a row of c terms: the longest
    chain of additions is one chunk plus the chunk adds (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2) and one
    rounding more for the weight 1 / c_t: tests/test_gpu_embed_grad.py's bound."""
    ref, mag = reference(k, dim)
    c = np.asarray(SIZES, dtype=np.float64)[TOUCHED]
    m = np.minimum(c, 512) + np.ceil(c / 512) + 1
    bound = (m * U / (1 - m * U))[:, None] * mag[TOUCHED]
    err = np.abs(out.double().cpu().numpy() - ref[TOUCHED])
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{what}: max |out - ref| = {err.max():.3e}, max err / bound = {worst:.3f}")
    assert np.all(err <= bound), f"{what}: |out - ref| exceeds gamma_m * sum|terms| (ratio {worst:.3f})"


def dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


@pytest.mark.parametrize("k", FANOUTS)
@pytest.mark.parametrize("dim", WIDTHS)
@pytest.mark.parametrize("placement", ["dense", "spread"])
def test_the_compact_gradient_is_the_dense_one_on_the_touched_rows(placement, dim, k):
    rows_n, m, nbr = placed(k, placement)
    cnt = case(k)[2]
    nbr_d, cnt_d = dev(nbr, cnt)
    g = grad_of(k, dim).to(DEV)
    rows, num, grad = ops.embed_grad_rows(g, nbr_d, cnt_d, rows_n)
    cap = min(nbr.size, rows_n)
    assert rows.shape == (cap,) and rows.dtype == torch.int32 and grad.shape == (cap, dim) and grad.dtype == torch.float32
    assert num.shape == (1,) and num.dtype == torch.int32 and int(num) == NU
    assert np.array_equal(rows[:NU].cpu().numpy(), m[TOUCHED]), "rows are not the ids with a run, ascending"
    dense = ops.embed_grad(g, nbr_d, cnt_d, rows_n)                                 # this placement's own dense gradient
    assert same_bits(grad[:NU], dense[rows[:NU].long()]), "a compact row differs from the row embed_grad stores"
    assert same_bits(grad[:NU], dense_rows(k, dim)), "the bits depend on where the ids lie in the table"
    check(grad[:NU], k, dim, f"{placement} dim {dim} k {k}")
    rows2, num2, grad2 = ops.embed_grad_rows(g, nbr_d, cnt_d, rows_n)
    assert int(num2) == NU and torch.equal(rows[:NU], rows2[:NU]) and same_bits(grad[:NU], grad2[:NU]), "two calls differ"


@pytest.mark.parametrize("k,dim", [(1, 4), (7, 52), (64, 128), (7, 132)])
def test_ids_up_to_2_31_cost_nothing(k, dim):
    """embed_rows = 2^31 - 1 with a run at 2^31 - 3: compact output only, in a workspace of exactly the size the query gives, which
    is the size it gives at embed_rows = n * k."""
    rows_n, m, nbr = placed(k, "huge")
    assert m[TOUCHED].max() == (1 << 31) - 3 and m.max() == (1 << 31) - 2
    cnt = case(k)[2]
    nbr_d, cnt_d = dev(nbr, cnt)
    need = ops.embed_grad_rows_workspace_bytes(nbr.shape[0], k, rows_n, dim)
    assert 0 < need == ops.embed_grad_rows_workspace_bytes(nbr.shape[0], k, nbr.size, dim)
    ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=DEV)
    rows, num, grad = ops.embed_grad_rows(grad_of(k, dim).to(DEV), nbr_d, cnt_d, rows_n, workspace=ws[:need])
    assert int(num) == NU and rows.shape[0] == nbr.size
    assert np.array_equal(rows[:NU].cpu().numpy().astype(np.int64), m[TOUCHED])
    assert same_bits(grad[:NU], dense_rows(k, dim))
    assert bool((ws[need:] == 0xA5).all()), "embed_grad_rows wrote past its workspace"


@pytest.mark.parametrize("k", FANOUTS)
@pytest.mark.parametrize("dim", [52, 128])
def test_the_bits_do_not_depend_on_where_the_sets_lie(dim, k):
    """The n rows of (nodes, nbr, cnt, grad_agg) permuted together, each layout summed in ops.row_order's order of its node ids."""
    rows_n, m, nbr = placed(k, "spread")
    nodes, _, cnt = case(k)
    g = grad_of(k, dim)
    n = len(cnt)
    nodes_d, nbr_d, cnt_d = dev(nodes, nbr, cnt)
    order = ops.row_order(nodes_d)
    ra, na, a = ops.embed_grad_rows(g.to(DEV), nbr_d, cnt_d, rows_n, row_order=order)
    assert int(na) == NU
    assert same_bits(a[:NU], ops.embed_grad(g.to(DEV), nbr_d, cnt_d, rows_n, row_order=order)[ra[:NU].long()])
    check(a[:NU], k, dim, f"row_order dim {dim} k {k}")
    perm = np.random.default_rng(5).permutation(n)
    nodes_p, nbr_p, cnt_p = dev(nodes[perm], nbr[perm], cnt[perm])
    rb, nb, b = ops.embed_grad_rows(g[torch.from_numpy(perm)].to(DEV), nbr_p, cnt_p, rows_n, row_order=ops.row_order(nodes_p))
    assert int(nb) == NU and torch.equal(ra[:NU], rb[:NU])
    assert same_bits(a[:NU], b[:NU]), f"{int((bits(a[:NU]) != bits(b[:NU])).sum())} elements differ between two layouts of the same sets"


@pytest.mark.parametrize("k,dim", [(7, 52), (64, 128)])
def test_sets_past_the_live_count_add_nothing(k, dim):
    """n_dev below n against the call on the truncated arrays, bit for bit; n_dev = 0 writes the count and nothing else."""
    rows_n, m, nbr = placed(k, "spread")
    cnt = case(k)[2]
    g = grad_of(k, dim).to(DEV)
    n = len(cnt)
    live = n - n // 3
    nbr_d, cnt_d = dev(nbr, cnt)
    n_dev = torch.tensor([live], dtype=torch.int32, device=DEV)
    rw, nw, want = ops.embed_grad_rows(g[:live].contiguous(), nbr_d[:live].contiguous(), cnt_d[:live].contiguous(), rows_n)
    rg, ng, got = ops.embed_grad_rows(g, nbr_d, cnt_d, rows_n, n_dev=n_dev)
    u = int(nw)
    assert 0 < u == int(ng) and torch.equal(rw[:u], rg[:u]) and same_bits(want[:u], got[:u])
    dense = ops.embed_grad(g, nbr_d, cnt_d, rows_n, n_dev=n_dev)
    assert same_bits(got[:u], dense[rg[:u].long()])
    full = ops.embed_grad_rows(g, nbr_d, cnt_d, rows_n)[2]
    assert not same_bits(got[:u], full[:u]), "the dead sets hold terms: the full call must differ"
    # no live set at all: U = 0, and neither the compact arrays nor the embedding are touched
    cap = 16
    rows_c = torch.full((cap,), -77, dtype=torch.int32, device=DEV)
    grad_c = torch.full((cap, dim), float("nan"), device=DEV)
    num_c = torch.full((1,), -5, dtype=torch.int32, device=DEV)
    embed = torch.full((rows_n, dim), 3.25, device=DEV)
    zero = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.embed_grad_rows(g, nbr_d, cnt_d, rows_n, n_dev=zero, max_rows=cap, embed=embed, lr=0.7, out=(rows_c, num_c, grad_c))
    assert int(num_c) == 0
    assert bool((rows_c == -77).all()) and bool(torch.isnan(grad_c).all()) and bool((embed == 3.25).all()), "a call without a live set wrote"
    # and the wrapper's own n == 0 path
    num_c.fill_(-5)
    ops.embed_grad_rows(g[:0], nbr_d[:0], cnt_d[:0], rows_n, max_rows=cap, embed=embed, lr=0.7, out=(rows_c, num_c, grad_c))
    assert int(num_c) == 0 and bool((rows_c == -77).all()) and bool((embed == 3.25).all())


def test_ids_are_clamped_into_the_embedding():
    """Ids below 0 and at or past embed_rows land on rows 0 and embed_rows - 1 (both without a term otherwise), which then lead and
    close the row list: rows and bits are those of the dense call on the same ids, and of the call on the clipped ids."""
    k, dim = 7, 52
    rows_n, m, nbr = placed(k, "spread")
    cnt = case(k)[2]
    g = grad_of(k, dim).to(DEV)
    bad = nbr.copy()
    assert cnt[0] == k and cnt[1] == k
    bad[0, 2], bad[1, 5], bad[1, 6] = -9, rows_n, np.iinfo(np.int32).max
    bad_d, clip_d, cnt_d = dev(bad, np.clip(bad, 0, rows_n - 1), cnt)
    padding = torch.from_numpy(nbr < 0).to(DEV)
    clip_d[padding] = -1                                                            # the padding slots stay padding
    rows, num, grad = ops.embed_grad_rows(g, bad_d, cnt_d, rows_n)
    u = int(num)
    assert NU < u <= NU + 2 and int(rows[0]) == 0 and int(rows[u - 1]) == rows_n - 1
    dense = ops.embed_grad(g, bad_d, cnt_d, rows_n)
    assert np.array_equal(rows[:u].cpu().numpy(), np.nonzero(dense.abs().sum(1).cpu().numpy())[0]), "rows are not the dense call's non-zero rows"
    assert same_bits(grad[:u], dense[rows[:u].long()])
    rows_c, num_c, grad_c = ops.embed_grad_rows(g, clip_d, cnt_d, rows_n)
    assert int(num_c) == u and torch.equal(rows[:u], rows_c[:u]) and same_bits(grad[:u], grad_c[:u])
    assert torch.equal(grad[0], g[0] * (1.0 / k))                                  # one term: fma(g, 1 / c, 0)


def fp64_update_check(new, old, g, lr, what):
    """|new - (old - lr g)| <= 2^-24 |old - lr g| (1 + 2^-20): one fp32 rounding of the exact value; the last factor covers the fp64
    reference's own rounding.  lr is the float32 the kernel is handed."""
    lr32 = float(np.float32(lr))
    ref = old.double() - lr32 * g.double()
    err = (new.double() - ref).abs()
    bound = U * ref.abs() * (1 + 2.0 ** -20)
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: max |new - ref| = {float(err.max()):.3e}, max err / bound = {worst:.3f}")
    assert bool((err <= bound).all()), f"{what}: more than one rounding away from old - lr * g (ratio {worst:.3f})"


@pytest.mark.parametrize("lr", [0.7, 0.0])
@pytest.mark.parametrize("k,dim,pad", [(7, 52, 4), (64, 128, 8), (1, 132, 4), (7, 4, 4)])
def test_the_update_touches_the_named_rows_once_and_nothing_else(k, dim, pad, lr):
    rows_n, m, nbr = placed(k, "spread")
    cnt = case(k)[2]
    nbr_d, cnt_d = dev(nbr, cnt)
    g = grad_of(k, dim).to(DEV)
    table = torch.full((rows_n, dim + pad), float("nan"), device=DEV)              # the canary in the padding columns
    table[:, :dim] = torch.randn(rows_n, dim, generator=torch.Generator().manual_seed(7)).to(DEV)
    old = table.clone()
    touched = torch.from_numpy(m[TOUCHED]).to(DEV)
    a = table.clone()
    ra, na, ga = ops.embed_grad_rows(g, nbr_d, cnt_d, rows_n, embed=a[:, :dim], lr=lr, want_grad=False)
    assert ra is None and ga is None and int(na) == NU
    b = table.clone()
    rb, nb, gb = ops.embed_grad_rows(g, nbr_d, cnt_d, rows_n, embed=b[:, :dim], lr=lr)
    assert int(nb) == NU and torch.equal(rb[:NU], touched.to(torch.int32))
    assert same_bits(gb[:NU], dense_rows(k, dim)), "the gradient returned beside the update is not the dense one"
    assert torch.equal(bits(a), bits(b)), "the update-only form and the form that also returns the gradient give different tables"
    mask = torch.zeros(rows_n, dtype=torch.bool, device=DEV)
    mask[touched] = True
    assert torch.equal(bits(a[~mask]), bits(old[~mask])), "a row that no term names was written"
    assert bool(torch.isnan(a[:, dim:]).all()), "the padding columns were written"
    fp64_update_check(a[touched, :dim], old[touched, :dim], dense_rows(k, dim), lr, f"dim {dim} k {k} lr {lr}")
    if lr == 0.0:
        assert torch.equal(bits(a), bits(old)), "lr = 0 must leave the table as it was"
    else:
        assert not bool((a[touched, :dim] == old[touched, :dim]).all()), "no touched row moved"


@pytest.mark.parametrize("k,dim", [(7, 52), (64, 128)])
def test_a_short_buffer_is_reported_and_respected(k, dim):
    """max_rows below U: the first max_rows rows are stored, the row behind them is not, U is still reported, and an update given in
    the same call still reaches all U rows."""
    rows_n, m, nbr = placed(k, "spread")
    cnt = case(k)[2]
    nbr_d, cnt_d = dev(nbr, cnt)
    g = grad_of(k, dim).to(DEV)
    pad = 4
    table = torch.randn(rows_n, dim, generator=torch.Generator().manual_seed(8)).to(DEV)
    full = table.clone()
    ops.embed_grad_rows(g, nbr_d, cnt_d, rows_n, embed=full, lr=0.7, want_grad=False)
    for cap in (1, NU - 1, NU):
        rows_c = torch.full((cap + 1,), -77, dtype=torch.int32, device=DEV)
        grad_c = torch.full((cap + 1, dim + pad), float("nan"), device=DEV)
        num_c = torch.zeros(1, dtype=torch.int32, device=DEV)
        t = table.clone()
        out = ops.embed_grad_rows(g, nbr_d, cnt_d, rows_n, max_rows=cap, embed=t, lr=0.7, out=(rows_c[:cap], num_c, grad_c[:cap, :dim]))
        assert out[1] is num_c and int(num_c) == NU, "U must be reported whatever the capacity"
        assert np.array_equal(rows_c[:cap].cpu().numpy(), m[TOUCHED][:cap])
        assert same_bits(grad_c[:cap, :dim], dense_rows(k, dim)[:cap])
        assert int(rows_c[cap]) == -77 and bool(torch.isnan(grad_c[cap]).all()), "something was written at row max_rows"
        assert bool(torch.isnan(grad_c[:, dim:]).all()), "columns [dim, ldr) were written"
        assert torch.equal(bits(t), bits(full)), "a short gradient buffer must not shorten the update"


def test_the_wrapper_refuses_what_does_not_fit():
    rows_n, m, nbr = placed(7, "dense")
    nbr_d, cnt_d = dev(nbr, case(7)[2])
    g = grad_of(7, 52).to(DEV)
    table = torch.zeros(R, 52, device=DEV)
    for kw in (dict(want_grad=False), dict(embed=table), dict(lr=0.5), dict(embed=torch.zeros(R, 56, device=DEV), lr=0.5),
               dict(embed=table[:R - 1], lr=0.5), dict(max_rows=0), dict(row_order=torch.zeros(3, dtype=torch.int32, device=DEV)),
               dict(out=(torch.zeros(3, dtype=torch.int32, device=DEV), None, None)),
               dict(out=(None, None, torch.zeros(R, 56, device=DEV)))):
        with pytest.raises(native.SageError):
            ops.embed_grad_rows(g, nbr_d, cnt_d, R, **kw)
    with pytest.raises(native.SageError):
        ops.embed_grad_rows(g[:10], nbr_d, cnt_d, R)
    with pytest.raises(native.SageError):
        ops.embed_grad_rows(g, nbr_d.long(), cnt_d, R)
