"""Shared helpers for the parity tests (fixtures -> tensors, tolerance)."""
import os

import numpy as np
import torch

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# *_b256: BASELINE configs[0] / configs[1] at their batch size (B = 256 seeds, full feature widths), the reference's own outputs
# (round 4; the table of such a fixture is regenerated from a committed integer seed, see synth_table / full_table)
TWO_LAYER_CASES_SMALL = ["tiny_gcn", "tiny_concat", "tiny_sigmoid", "cora_emb_gcn_5_5", "cora_emb_concat_10_10",
                         "cora_bow_gcn_5_5", "cora_bow_concat_5_5", "pubmed_gcn_10_25", "pubmed_concat_10_25"]
TWO_LAYER_CASES_B256 = ["cora_gcn_10_10_b256", "cora_concat_10_10_b256", "cora_gcn_5_5_b256", "cora_concat_5_5_b256",
                        "pubmed_gcn_10_25_b256", "pubmed_concat_10_25_b256"]
TWO_LAYER_CASES = TWO_LAYER_CASES_SMALL + TWO_LAYER_CASES_B256

# BASELINE.json north_star: "within 1e-5 relative fp32".  SURVEY.md section 7 (Tolerance
# definition): the reference's own fp32 result is only reproducible relative to the row
# maximum, so |a-b| <= RTOL * max|ref row| (+ rtol elementwise) is the gate everywhere.
RTOL = 1e-5


def load_golden(name):
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


TABLE_KINDS = {0: "bow", 1: "tfidf"}


def synth_table(kind, n, d, seed):
    """Feature tables of the batch-size fixtures, a pure function of (kind, n, d, seed) -- shared with tests/golden/make_golden.py, which
    records the sha256 of the bytes it fed to the reference.  bow: Cora-like 0/1 bag of words (18 words of 1433 per paper on average);
    tfidf: SURVEY 8(d)'s Pubmed stand-in, rand * Bernoulli(0.1)."""
    rng = np.random.default_rng(int(seed))
    if kind == "bow":
        return (rng.random((n, d)) < 18.0 / d).astype(np.float32)
    if kind == "tfidf":
        return (rng.random((n, d)) * (rng.random((n, d)) < 0.1)).astype(np.float32)
    raise ValueError(kind)


def full_table(g):
    """Rebuild the [N, D0] table: a small fixture stores the touched rows, a batch-size fixture the generator's (kind, seed) and
    the checksum of the table the reference saw."""
    if "table_kind" in g:
        import hashlib
        t = synth_table(TABLE_KINDS[int(g["table_kind"])], int(g["num_nodes"]), int(g["d0"]), int(g["table_seed"]))
        digest = np.frombuffer(hashlib.sha256(t.tobytes()).digest(), dtype=np.uint8)
        assert np.array_equal(digest, g["table_sha256"]), "regenerated feature table differs from the one the reference was run on"
        return torch.from_numpy(t)
    t = torch.zeros(int(g["num_nodes"]), int(g["d0"]))
    t[torch.from_numpy(g["feat_ids"])] = torch.from_numpy(g["feat_rows"])
    return t


def assert_agg1_close(actual, g, what="agg1_out"):
    """Layer-1 aggregator output against the fixture: all rows (small fixtures), or the recorded sample of rows (batch-size
    fixtures keep 16 of the [|S1|, D0] rows: the whole matrix is 7 MB at Cora's width)."""
    if "agg1_out" in g:
        return assert_close_rowmax(actual, g["agg1_out"], what=what)
    rows = torch.from_numpy(g["agg1_rows"])
    return assert_close_rowmax(torch.as_tensor(np.asarray(actual))[rows], g["agg1_out_rows"], what=what + " (row sample)")


def sets_from_padded(nodes, nbr, cnt):
    return {int(n): set(int(x) for x in nbr[r, :int(cnt[r])]) for r, n in enumerate(nodes)}


def torch_two_hop(table, w1, w2, g):
    """The reference's expression (aggregators.py:54-74, encoders.py:49-62) on the fixture's injected sets, differentiable, fp64."""
    gcn = bool(g["gcn"])
    l1 = torch.from_numpy(g["layer1_nodes"])
    pos = {int(v): i for i, v in enumerate(g["layer1_nodes"])}

    def mean_rows(src, nbr, cnt, index_of):
        rows = []
        for r in range(nbr.shape[0]):
            ids = [index_of(int(x)) for x in nbr[r, :int(cnt[r])]]
            rows.append(src[ids].mean(0))
        return torch.stack(rows)

    agg1 = mean_rows(table, g["nbr1"], g["cnt1"], lambda x: x)
    x1 = agg1 if gcn else torch.cat([table[l1], agg1], 1)
    h1 = torch.relu(x1 @ w1.t())
    agg2 = mean_rows(h1, g["nbr2"], g["cnt2"], lambda x: pos[x])
    x2 = agg2 if gcn else torch.cat([h1[[pos[int(s)] for s in g["seeds"]]], agg2], 1)
    return torch.relu(x2 @ w2.t())                     # [B, H2]


def oracle_on_engine_sets(eng, table, w1, w2, seeds):
    """The fp64 oracle (ref_sparse.two_hop_forward) on the sets of `eng`'s LAST forward, read back from its workspace.  table / w1 / w2:
    the caller's tensors, seeds: the caller's ids.  A relabelled engine's sets hold INTERNAL ids: the table is taken in internal order
    (table[node_order]) and the seeds are mapped to internal ids; the rows stay in the caller's seed order.  -> [B, H2] float64."""
    from oracle import ref_sparse
    it = eng.intermediates()
    first = it["first_frontier_row"]
    s1, nbr1, cnt1 = it["s1_nodes"].cpu().numpy(), it["nbr1"].cpu().numpy(), it["cnt1"].cpu().numpy()
    nbr2, cnt2 = it["nbr2"].cpu().numpy(), it["cnt2"].cpu().numpy()
    t = table.detach().cpu()
    seeds = np.asarray(seeds, dtype=np.int64)
    if eng.node_order is not None:
        t = t[eng.node_order.cpu()]
        seeds = eng._new_of_old.cpu().numpy().astype(np.int64)[seeds]
    if eng.concat:
        assert np.array_equal(s1[:first], seeds)
    return ref_sparse.two_hop_forward(t, w1.detach().cpu(), w2.detach().cpu(), seeds, nbr2, cnt2, s1[first:], nbr1[first:], cnt1[first:],
                                      gcn=not eng.concat, agg_gcn=eng.agg_self_loop, seed_nbr1=nbr1[:first] if eng.concat else None,
                                      seed_cnt1=cnt1[:first] if eng.concat else None)


def assert_close_rowmax(actual, expected, rtol=RTOL, rows_dim=0, what=""):
    """|a-b| <= rtol * max|expected row|; NaNs must coincide."""
    a = torch.as_tensor(np.asarray(actual), dtype=torch.float64)
    e = torch.as_tensor(np.asarray(expected), dtype=torch.float64)
    assert a.shape == e.shape, f"{what}: shape {tuple(a.shape)} vs {tuple(e.shape)}"
    if rows_dim == 1:
        a, e = a.t(), e.t()
    nan_a, nan_e = torch.isnan(a), torch.isnan(e)
    assert torch.equal(nan_a, nan_e), f"{what}: NaN pattern differs"
    a = torch.nan_to_num(a)
    e = torch.nan_to_num(e)
    if e.numel() == 0:
        return 0.0
    scale = e.abs().amax(dim=1, keepdim=True).clamp_min(1e-30)
    err = ((a - e).abs() / scale).max().item()
    assert err <= rtol, f"{what}: max |a-b|/rowmax = {err:.3e} > {rtol:.1e}"
    return err


def usable_cores():
    """Host cores this process may actually use: the affinity mask / cgroup quota, not the machine's core count (a GPU box
    reports 256 cores to a 16-core share, and torch's CPU ops on 256 intra-op threads run 20x slower there than on 16)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = max(1, min(n, int(int(quota) / int(period))))
    except Exception:
        pass
    return n


# ------------------------------------------------------------------------------------------------------------------------------
# The split layer 1 (csrc/sage_gather.hip + dense_bf16x3_kernel of csrc/sage_dense.hip): data generators, fp64 references and the
# two element-wise bars, shared by tests/test_gpu_split_layer1.py (the kernels) and tests/test_split_layer1_host.py (numpy fp32
# emulations of the kernels' arithmetic, faithful and deliberately broken, on the very same data).
def gather_form(dim, ld, ldo, n, k, aligned=True):
    """sage_launch_gather_mean's default dispatch on a row-major table, restated: -> (form, lanes per slice, ids per trip).
    "sliced": the column-sliced pipelined kernel (16-lane slices; ONE 32-lane slice for rows of at most 128 floats that do not
    end on a 64-float boundary), U = 2 / 4 / 8 wave-instructions of 64 / lanes ids per trip; "wave4" / "wave1": one wave per
    row with 16-byte or 4-byte loads, 8 row loads in flight, ids in pages of 64."""
    vec4 = dim % 4 == 0 and ld % 4 == 0 and ldo % 4 == 0 and aligned
    if vec4 and k <= 64 and ((dim >= 64 and n >= 8192) or dim > 256):
        sl = 32 if (dim <= 128 and dim % 64 != 0) else 16
        per = 64 // sl
        need = -(-k // per)
        u = (4 if need <= 4 else 8) if sl == 32 else (2 if need <= 2 else 4 if need <= 4 else 8)
        return "sliced", sl, per * u
    return ("wave4" if vec4 else "wave1"), 64, 8


def edge_counts(k, trip):
    """List lengths for a fanout of k: k, 0, 1, k - 1 and one short of, on and one past every multiple of `trip` (and of 64)."""
    vals = [k, 0, 1, k - 1]
    for step in (trip, 64):
        for b in range(step, k + 2, step):
            vals += [b - 1, b, b + 1]
    out = []
    for v in vals:
        if 0 <= v <= k and v not in out:
            out.append(v)
    return out


GATHER_HEAVY = 8          # table rows [0, 8) carry 64 x the magnitude of the others; every list ends in one of them


def gather_case(n, k, dim, trip, seed):
    """Hand-made inputs of one gather_mean call (numpy; ids are table rows).
    cnt cycles through edge_counts(k, trip).  Row r's self row, by (r % L + r // L) % 6 with L list lengths (every length meets every kind): none; a row that is not in the list; list[0]; the
    last valid entry; an entry in a trip after the first (cycling through the trips); an entry at a position >= 64 where the list
    is that long (else the entry before the last).  Lists hold distinct ordinary rows and end (last VALID entry) in a heavy row.
    Values: 10^U(-6, -1) with random signs, 10^U(-1, 0) in a row's last four columns, x 64 in the heavy rows."""
    rs = np.random.default_rng(seed)
    pool = max(k + 3, 61)
    P = GATHER_HEAVY + pool
    T = P + 2                                                     # + an ordinary and a heavy row that no list holds
    mag = 10.0 ** rs.uniform(-6, -1, (T, dim))
    mag[:, max(dim - 4, 0):] = 10.0 ** rs.uniform(-1, 0, (T, min(dim, 4)))
    mag[:GATHER_HEAVY] *= 64
    mag[P + 1] *= 64
    table = (mag * rs.choice([-1.0, 1.0], (T, dim))).astype(np.float32)
    vals = edge_counts(k, trip)
    r = np.arange(n)
    cnt = np.asarray(vals)[r % len(vals)].astype(np.int64)
    nbr = (np.argsort(rs.random((n, pool)), axis=1)[:, :k] + GATHER_HEAVY).astype(np.int64)
    has = cnt > 0
    nbr[r[has], cnt[has] - 1] = r[has] % GATHER_HEAVY
    mode = (r % len(vals) + r // len(vals)) % 6
    mode[1:2] = 0                                                 # row 1 (cnt = 0) has no self row: an empty set even when n = 2
    long = np.nonzero(cnt > 64)[0]
    mode[long[1::2]] = 5                                          # every second list longer than 64: a self row at a position >= 64
    ntrip_after = np.maximum((cnt - 1) // trip, 1)
    pos4 = np.where(cnt > trip, np.minimum((1 + (r // 6) % ntrip_after) * trip + r % trip, cnt - 1), cnt // 2)
    pos5 = np.where(cnt > 64, 64 + r % np.maximum(cnt - 64, 1), np.maximum(cnt - 2, 0))
    pos = np.select([mode == 2, mode == 3, mode == 4, mode == 5], [0 * r, np.maximum(cnt - 1, 0), pos4, pos5], 0)
    absent = P + r % 2
    self_eff = np.where(mode == 0, -1, np.where((mode == 1) | ~has, absent, nbr[r, np.minimum(pos, k - 1)]))
    return {"table": table, "nbr": nbr, "cnt": cnt, "self": self_eff.astype(np.int64), "pos": pos, "mode": mode, "trip": trip}


def gather_reference(table, nbr, cnt, self_eff, flag):
    """fp64 mean over the set (list[:cnt] and, unless it is among them, the self row) -> (ref, bar, ceff).  Empty sets: NaN when
    `flag`, zeros otherwise.  bar = 1.01 (ceff + 2) 2^-24 sum_j |x_j| / ceff per element: an fp32 sum of ceff terms in any order
    ((ceff - 1) roundings of at most 2^-24 of the sum of magnitudes each) times a rounded reciprocal, rounded (2 more), with 1 %
    for the second-order terms.  Derived, not measured."""
    t = np.asarray(table, dtype=np.float64)
    n, k = nbr.shape
    tot, mass = np.zeros((n, t.shape[1])), np.zeros((n, t.shape[1]))
    inlist = np.zeros(n, dtype=bool)
    for j in range(k):
        m = j < cnt
        rows = t[np.clip(nbr[:, j], 0, len(t) - 1)] * m[:, None]
        tot += rows
        mass += np.abs(rows)
        if self_eff is not None:
            inlist |= m & (nbr[:, j] == self_eff)
    extra = np.zeros(n, dtype=bool) if self_eff is None else (self_eff >= 0) & ~inlist
    if extra.any():
        srow = t[np.clip(self_eff, 0, len(t) - 1)] * extra[:, None]
        tot += srow
        mass += np.abs(srow)
    ceff = cnt + extra
    d = np.maximum(ceff, 1)[:, None]
    ref = tot / d
    ref[ceff == 0] = np.nan if flag else 0.0
    bar = 1.01 * (ceff[:, None] + 2) * 2.0 ** -24 * mass / d
    return ref, bar, ceff


def gather_miss(got, ref, bar, ceff):
    """How `got` misses the gather bar: None when it meets it, else a message.  NaN and zero fills of empty sets must coincide
    exactly; every other element is within its bar."""
    got = np.asarray(got, dtype=np.float64)
    if got.shape != ref.shape:
        return f"shape {got.shape} vs {ref.shape}"
    if not np.array_equal(np.isnan(got), np.isnan(ref)):
        return f"NaN pattern differs in rows {np.nonzero((np.isnan(got) != np.isnan(ref)).any(1))[0][:8].tolist()}"
    empty = ceff == 0
    if empty.any() and not np.isnan(ref[empty]).any() and np.any(got[empty] != 0.0):
        return "an empty set is not filled with zeros"
    fin = ~np.isnan(ref)
    excess = np.where(fin, np.abs(np.where(fin, got - ref, 0.0)) - bar, -1.0)
    if np.any(excess > 0):
        r, c = np.unravel_index(np.argmax(np.where(fin, np.abs(np.where(fin, got - ref, 0.0)) / np.maximum(bar, 1e-300), 0.0)), ref.shape)
        return (f"row {r} (set of {ceff[r]}) column {c}: |got - ref| = {abs(got[r, c] - ref[r, c]):.3e} > bar {bar[r, c]:.3e} "
                f"({int((excess > 0).sum())} elements over)")
    return None


def split_graph(rows, k1, concat, self_loop, seed):
    """A hand-made seed -> frontier graph for `rows` layer-1 rows, whose degrees are at most the fanouts (k1 inner, 64 outer), so the
    sampler takes whole neighbourhoods.  With an outer fanout of 64 one wavefront samples one seed and the seed's neighbours get
    consecutive frontier rows in list order; only the order of the seeds' CHUNKS is the device's choice.  So every chunk ends alike --
    ..., a row that takes the contraction's exact path, a row that carries the largest values -- and whichever chunk comes last, the
    last layer-1 row and the last 32-row tile are what the test wants them to be.
    Layer-1 rows: gcn: the frontier, chunks of 64; gcn with the self-loop aggregator: chunks of up to 63 frontier nodes followed by
    their seed; concat: the seeds in order, then the frontier (one node below 100 rows, a third of the rows above).
    Nodes: seeds [0, b), frontier [b, b + f), one private node per seed / frontier node, then 72 shared pool nodes.  Inner hop: node
    v's list is c_v - 1 pool nodes and, last, its private node (under the self-loop aggregator a list of one is [v] itself, and every
    third longer list holds v in the middle: the set union must not count it twice); c_v cycles through 1, k1, k1 - 1 and the values
    around every multiple of 8.  `ender`: the nodes whose rows end a chunk (concat without a frontier: the last seed); `huge`: the
    nodes before them (concat with at most one frontier node: the last seed), with a list of one; `iso`: one node without
    neighbours, 13 rows into the first chunk (concat: seed 13, or an earlier one), -1 when there are too few rows.
    `order`: the layer-1 rows with the chunks in seed order."""
    if concat:
        f = (0 if rows == 1 else 1) if rows < 100 else rows // 3
        b = rows - f
        sizes = [64] * (f // 64) + ([f % 64] if f % 64 else [])
    elif self_loop:
        b = -(-rows // 64)
        f = rows - b
        sizes = [min(63, max(f - 63 * i, 0)) for i in range(b)]
    else:
        f = rows
        sizes = [64] * (f // 64) + ([f % 64] if f % 64 else [])
        b = len(sizes)
    assert len(sizes) <= b and sum(sizes) == f
    nl = b + f
    pool0, npool = 2 * nl, 72
    N = pool0 + npool
    starts = b + np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    chunks = [np.arange(starts[i], starts[i] + sizes[i]) for i in range(len(sizes))]
    ender, huge, mate, order = [], [], {}, []
    for i, ch in enumerate(chunks):
        members = list(ch) + ([i] if self_loop else [])
        order += members
        if members:
            ender.append(int(members[-1]))
            mate[int(members[-1])] = int(members[-2]) if len(members) >= 2 else -1
            if len(members) >= 2:
                huge.append(int(members[-2]))
    if concat:
        order = list(range(b)) + order
        if f == 0:
            ender.append(b - 1)
            mate[b - 1] = -1
        elif f == 1 and b >= 2:
            huge.append(b - 1)
            mate[ender[-1]] = b - 1
    iso = -1
    if rows >= 3:
        if concat:
            iso = min(13, b - 2) if b >= 3 else -1
        elif sizes[0] >= 16:
            iso = int(chunks[0][13])
        elif sizes[0] >= 3:
            iso = int(chunks[0][0])
    vals = [v for v in edge_counts(k1, 8) if v >= 1]
    deg = np.zeros(N, dtype=np.int64)
    deg[:nl] = np.asarray(vals)[(np.arange(nl) * 5 + seed) % len(vals)]
    deg[huge] = 1
    if iso >= 0:
        deg[iso] = 0
    rowptr_in = np.zeros(N + 1, dtype=np.int64)
    rowptr_in[1:] = np.cumsum(deg)
    col_in = np.zeros(int(rowptr_in[-1]), dtype=np.int32)
    v = np.repeat(np.arange(nl), deg[:nl])
    j = np.arange(len(col_in)) - rowptr_in[v]
    col_in[:] = pool0 + (v * 7 + j) % npool                      # distinct for j < 72
    last = j == deg[v] - 1
    src = nl + np.arange(nl)
    if self_loop:
        src[deg[:nl] == 1] = np.nonzero(deg[:nl] == 1)[0]
        mid = (j == deg[v] // 2) & (v % 3 == 0) & (deg[v] >= 3)
        col_in[mid] = v[mid]
    col_in[last] = src[v[last]]
    od = np.zeros(N, dtype=np.int64)
    od[:len(sizes)] = sizes
    rowptr_out = np.zeros(N + 1, dtype=np.int64)
    rowptr_out[1:] = np.cumsum(od)
    col_out = (b + np.arange(f)).astype(np.int32)
    return {"num_nodes": N, "rowptr_in": rowptr_in, "col_in": col_in, "rowptr_out": rowptr_out, "col_out": col_out, "deg": deg,
            "src": src, "iso": iso, "nl": nl, "b": b, "f": f, "ender": ender, "huge": huge, "mate": mate,
            "order": np.asarray(order, dtype=np.int64)}


def split_lists(g, s1_nodes, k1):
    """The padded inner-hop lists of layer-1 rows `s1_nodes` of split_graph `g`, in CSR order: what a sampler that takes whole
    neighbourhoods leaves (as sets).  -> (nbr1 [rows, k1], cnt1 [rows])"""
    s1 = np.asarray(s1_nodes, dtype=np.int64)
    cnt1 = g["deg"][s1]
    nbr1 = np.zeros((len(s1), k1), dtype=np.int64)
    for j in range(k1):
        m = j < cnt1
        nbr1[m, j] = g["col_in"][g["rowptr_in"][s1[m]] + j]
    return nbr1, cnt1


def split_data(g, d0, h1, concat, seed):
    """Table [N, d0] and W1 [h1, m d0] for split_graph `g`.  Values 10^U(-2, 0) with random signs; the last four columns of the
    table and of each K chunk of W1 x 16 (the last four K columns carry the largest products), the rows that end a list x 4, the
    `ender` nodes' list-ending rows x 8 x the list's length more (and, concat, their own rows x 8), W1's last output row x 8.
    The `huge` nodes get a 3e38 entry in column 1 -- concat: of their own table row; gcn: of the row that IS their one-entry list --
    so that their rows alone take the contraction's exact path (that K column of W1 is divided by 64: no product overflows).
    -> (table, w1)"""
    rs = np.random.default_rng(seed)
    N, nl = g["num_nodes"], g["nl"]
    m = 2 if concat else 1
    table = 10.0 ** rs.uniform(-2, 0, (N, d0)) * rs.choice([-1.0, 1.0], (N, d0))
    table[:, d0 - 4:] *= 16
    table[np.unique(g["src"])] *= 4
    for e in g["ender"]:
        table[g["src"][e]] *= 8 * max(int(g["deg"][e]), 1)
        if concat and g["src"][e] != e:
            table[e] *= 8
    w1 = rs.standard_normal((h1, m * d0)) / np.sqrt(m * d0)
    for c in range(m):
        w1[:, (c + 1) * d0 - 4: (c + 1) * d0] *= 16
    w1[-1] *= 8
    for h in g["huge"]:
        table[h if concat else g["src"][h], 1] = 3.0e38
    w1[:, 1 if concat else (m - 1) * d0 + 1] /= 64
    return table.astype(np.float32), w1.astype(np.float32)


def contraction_units(got, x, w):
    """|got - x . w^T| per element in units of 2^-23 sum_k |x_k||w_k| (x, w: what the kernel was given, fp32), against fp64.
    Rows of x that hold a NaN are NaN rows of the reference.  -> (units [n, h], ref)"""
    x64, w64 = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    nanrow = np.isnan(x64).any(1)
    xz = np.where(nanrow[:, None], 0.0, x64)
    ref = xz @ w64.T
    scale = 2.0 ** -23 * (np.abs(xz) @ np.abs(w64).T)
    units = np.abs(np.asarray(got, dtype=np.float64) - ref) / np.maximum(scale, 1e-300)
    ref[nanrow] = np.nan
    units[nanrow] = 0.0
    return units, ref


def contraction_bar(x, w, concat):
    """The bar of the split-bf16 contraction in units of 2^-23 sum_k |x_k||w_k|.  K <= 512: the project's own figures for this
    kernel (tests/test_gpu_round2.py: 4 for the gcn encoder, 6 for concat); deeper K (nobody has measured the multi-pass kernel): 6.
    Or twice what torch's fp32 mm leaves on the same data on the CPU, whichever is larger -- the torch-fp32 yardstick, not derived.
    -> (bar, torch's own figure)"""
    fin = ~np.isnan(np.asarray(x)).any(1)
    xf, wf = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32)[fin])), torch.from_numpy(np.asarray(w, dtype=np.float32))
    e_torch = float(contraction_units((xf @ wf.t()).numpy(), xf.numpy(), wf.numpy())[0].max()) if fin.any() else 0.0
    base = (6.0 if concat else 4.0) if x.shape[1] <= 512 else 6.0
    return max(base, 2.0 * e_torch), e_torch


# ------------------------------------------------------------------------------------------------------------------------------
# The generic contraction linear_act_kernel (csrc/sage_linear.hip): cases, data, a numpy fp32 emulation of its accumulation and
# masks, and the bar -- shared by tests/test_gpu_linear_act.py (the kernel) and tests/test_linear_act_host.py (the emulation,
# faithful and deliberately broken, on the very same data).
LINEAR_MODES = ("gcn", "concat", "concat_index")      # no self_tab; self_tab row r for output row r; self_tab row self_index[r]

# (n, dim, out_dim, small n_dev or None): every n, dim and out_dim the kernel's masks distinguish -- the 64-row tile with its two
# 32-row accumulators, four waves of 32 columns, 128-column blocks in grid.y, 32-wide K panels -- and each out_dim with an n that is
# no multiple of 32.  Each shape runs in all three modes, without n_dev and with n_dev = max(n - 3, 0); a small n_dev in addition
# leaves whole 64-row tiles empty.  dim = 1433 (K = 1433 gcn, 2866 concat: the deepest in use) at n = 65 only.
LINEAR_SHAPES = [
    (1, 1, 1, None),
    (31, 7, 3, None),
    (33, 31, 31, None),
    (63, 32, 32, None),
    (65, 33, 33, None),
    (129, 50, 50, None),
    (31, 64, 96, None),
    (33, 100, 97, None),
    (63, 1, 127, None),
    (65, 7, 128, None),
    (129, 31, 129, None),
    (1, 33, 300, None),
    (32, 50, 33, None),
    (64, 64, 50, None),
    (129, 100, 300, 40),
    (65, 1433, 128, None),
]
LINEAR_RUNS = [(n, dim, h, mode, small) for (n, dim, h, small) in LINEAR_SHAPES for mode in LINEAR_MODES]


def linear_n_devs(n, small):
    """The device-side row counts a shape runs with: absent, n - 3 (0 at n < 3: the only tile is empty) and the small one."""
    return [None, max(n - 3, 0)] + ([small] if small is not None else [])


def linear_case(n, dim, out_dim, mode, seed=0):
    """Hand-made inputs of one linear_act call as the kernel sees them: flat fp32 allocations (numpy) with every operand a view
    ("agg", "self", "w", "out": (offset, ld) into the allocation of the same name + "_flat"), based one float in, with odd pads --
    ld_agg = dim + 1, ld_self = dim + 3, ldw = 2 dim + 5, ldo = out_dim + 3 -- and one spare row behind each.  W is allocated as
    the concat W [out_dim, 2 dim]; the gcn mode's W is its agg half, the view W[:, dim:] (same ld).  Every entry, pads included, is
    +-U[0.5, 1): each of the K terms of an output is at least 1 / (4 K) of sum |x||w|, and a read that strays into a pad finds a
    finite value of the same size.  concat_index: the table has n + 3 rows, self_index is a permutation of the first n + 2 without
    a fixed point in [0, n), and the last row, which no index names, is NaN."""
    assert mode in LINEAR_MODES
    rs = np.random.default_rng(1000 * n + 10 * dim + out_dim + seed)

    def flat(size):
        return (rs.uniform(0.5, 1.0, size) * rs.choice([-1.0, 1.0], size)).astype(np.float32)

    ld_agg, ld_self, ldw, ldo = dim + 1, dim + 3, 2 * dim + 5, out_dim + 3
    tab_rows = n + 3 if mode == "concat_index" else n
    c = {"n": n, "dim": dim, "out_dim": out_dim, "mode": mode, "tab_rows": tab_rows,
         "agg_flat": flat(1 + ld_agg * (n + 1)), "agg": (1, ld_agg),
         "self_flat": flat(1 + ld_self * (tab_rows + 1)), "self": (1, ld_self) if mode != "gcn" else None,
         "w_flat": flat(1 + ldw * (out_dim + 1)), "w": (1 + (dim if mode == "gcn" else 0), ldw),
         "out": (1, ldo), "out_size": 1 + ldo * (n + 1), "self_index": None}
    if mode == "concat_index":
        while True:
            perm = rs.permutation(n + 2)
            if not np.any(perm[:n] == np.arange(n)):
                break
        c["self_index"] = perm[:n].astype(np.int64)
        off, ld = c["self"]
        c["self_flat"][off + ld * (n + 2): off + ld * (n + 2) + dim] = np.nan
    return c


def linear_poisoned(c, n_dev):
    """The case as it is run with a device-side row count: rows of agg (and, without self_index, of self_tab) at or past n_dev are
    NaN, entries of self_index at or past n_dev name the spare NaN row of the table.  A copy; `c` is left alone."""
    p = dict(c)
    n, dim = c["n"], c["dim"]
    p["agg_flat"] = c["agg_flat"].copy()
    off, ld = c["agg"]
    for r in range(n_dev, n):
        p["agg_flat"][off + r * ld: off + r * ld + dim] = np.nan
    if c["mode"] == "concat":
        p["self_flat"] = c["self_flat"].copy()
        off, ld = c["self"]
        for r in range(n_dev, n):
            p["self_flat"][off + r * ld: off + r * ld + dim] = np.nan
    if c["mode"] == "concat_index":
        p["self_index"] = c["self_index"].copy()
        p["self_index"][n_dev:] = n + 2
    return p


def linear_view(c, name, rows, cols):
    """The [rows, cols] operand `name` of a case, a copy"""
    off, ld = c[name]
    return c[name + "_flat"][off + ld * np.arange(rows)[:, None] + np.arange(cols)[None, :]]


def linear_operands(c):
    """-> (x [n, K], w [out_dim, K]): the [self | agg] rows and the weight rows that the call's arguments name."""
    n, dim = c["n"], c["dim"]
    agg = linear_view(c, "agg", n, dim)
    k = dim * (1 if c["mode"] == "gcn" else 2)
    w = linear_view(c, "w", c["out_dim"], k)
    if c["mode"] == "gcn":
        return agg, w
    tab = linear_view(c, "self", c["tab_rows"], dim)
    own = tab[:n] if c["self_index"] is None else tab[c["self_index"]]
    return np.concatenate([own, agg], 1), w


def bf16_round(x):
    """fp32 -> the nearest bf16 (ties to even), as fp32"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    u = (u + (((u >> 16) & 1) + np.uint32(0x7FFF))) & np.uint32(0xFFFF0000)
    return u.view(np.float32)


LINEAR_VARIANTS = ("fma", "mul_add")
LINEAR_BROKEN = ("drop_k", "seam", "self_row", "k_tail", "bf16")


def linear_broken_applies(broken, c):
    """Does this defect change what the kernel computes at this case?  The seam and the self row exist in the concat modes, the K
    tail where K is no multiple of the 32-wide panel."""
    k = c["dim"] * (1 if c["mode"] == "gcn" else 2)
    return {"drop_k": True, "bf16": True, "seam": c["mode"] != "gcn", "self_row": c["mode"] == "concat_index", "k_tail": k % 32 != 0}[broken]


def linear_act_emulate(c, nn=None, variant="fma", broken=None, fill=np.nan):
    """linear_act_kernel's pre-activation in numpy fp32, loads, masks and order as the kernel has them: 32-wide K panels, panel column
    gk < ds from self_tab row self_index[r] (or r), the rest from agg column gk - ds, rows at or past nn and columns at or past K
    zero, W rows likewise; k ascending, two terms per matrix instruction.  The instruction's rounding is not documented, so there
    are two variants: "fma", acc = fma(a1, b1, fma(a0, b0, acc)), and "mul_add", both products rounded to fp32 and added to acc one
    after the other.  Rows at or past nn are not stored: they hold `fill`.  -> [n, out_dim] fp32.
    broken: "drop_k" leaves out the term k = K // 2; "seam" puts the seam one column early (panel column ds - 1 is read from agg
    column -1); "self_row" reads self_tab row r where self_index[r] is meant; "k_tail" does not mask the panel columns at or past K
    (both operands read on past their rows); "bf16" rounds the row operand to bf16."""
    n, dim, h = c["n"], c["dim"], c["out_dim"]
    nn = n if nn is None else min(nn, n)
    ds = 0 if c["self"] is None else dim
    K = ds + dim
    kp = -(-K // 32) * 32
    gk = np.arange(kp)
    rows = np.arange(n)

    def load(name, r, col):
        off, ld = c[name]
        buf = c[name + "_flat"]
        return buf[np.clip(off + ld * r[:, None] + col[None, :], 0, len(buf) - 1)]

    kmask = np.ones(kp, dtype=bool) if broken == "k_tail" else gk < K
    seam = ds - 1 if (broken == "seam" and ds) else ds
    a = np.zeros((n, kp), dtype=np.float32)
    if ds:
        sr = c["self_index"] if (c["self_index"] is not None and broken != "self_row") else rows
        a[:, :seam] = load("self", sr, gk[:seam])
    a[:, seam:] = load("agg", rows, gk[seam:] - ds)
    a[:, ~kmask] = 0
    a[nn:] = 0
    b = load("w", np.arange(h), gk)
    b[:, ~kmask] = 0
    if broken == "drop_k":
        a[:, K // 2] = 0
    if broken == "bf16":
        a = bf16_round(a)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    acc = np.zeros((n, h), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(kp):
            p = a64[:, k, None] * b64[None, :, k]                # an fp32 x fp32 product is exact in fp64
            if variant == "mul_add":
                p = p.astype(np.float32).astype(np.float64)
            acc = (acc.astype(np.float64) + p).astype(np.float32)
    out = np.full((n, h), fill, dtype=np.float32)
    out[:nn] = acc[:nn]
    return out


def linear_bar(c, nn=None):
    """The bar of the generic contraction on one case, in units of 2^-23 sum_k |x_k||w_k| per element: twice the worst figure that
    either variant of the emulation leaves on the same data (NOT a figure of the kernel) -- the margin of 2 because nobody has
    measured how v_mfma_f32_32x32x2_f32 rounds its two-term step; both variants measured 0.5 to 1.8 units on this kind of data for
    K from 1 to 2866.  And the condition under which that bar has teeth: the smallest single term's share of an output,
    min over (row, column, k) of |x_k w_k| in the same units, of which the bar must stay below one eighth.
    Rows at or past nn are left out.  -> (bar, {variant: figure}, share)"""
    n = c["n"] if nn is None else min(nn, c["n"])
    x, w = linear_operands(c)
    x, w = x[:n], w
    if n == 0:
        return 0.0, {v: 0.0 for v in LINEAR_VARIANTS}, np.inf
    figs = {}
    for v in LINEAR_VARIANTS:
        got = linear_act_emulate(c, nn=nn, variant=v)[:n]
        figs[v] = float(contraction_units(got, x, w)[0].max())
    ax, aw = np.abs(x.astype(np.float64)), np.abs(w.astype(np.float64))
    smallest = np.full((n, w.shape[0]), np.inf)
    for k in range(x.shape[1]):
        smallest = np.minimum(smallest, ax[:, k, None] * aw[None, :, k])
    share = float((smallest / (2.0 ** -23 * (ax @ aw.T))).min())
    return 2.0 * max(figs.values()), figs, share


# ------------------------------------------------------------------------------------------------------------------------------
# The CSR chunk planner (csrc/sage_csr_common.h: csr_count_kernel -> csr_carry_kernel -> csr_expand_kernel, then chunk_item and
# chunked_row_sum): cases whose long rows sit where the count scan changes thread, wave, block and carry pass, a numpy emulation of the
# three launches (faithful and deliberately broken), fp64 references with derived per-element bars, and an fp32 emulation of what a
# row comes out as under a given plan -- shared by tests/test_gpu_csr_plan.py (the kernels) and tests/test_csr_plan_host.py (the
# emulations on the very same data).
# The geometry, as sage_csr_common.h has it (kCountIpt, kWave, kCountThreads, kCountTile, kCarryThreads, kChunk):
PLAN_IPT, PLAN_WAVE, PLAN_THREADS = 8, 64, 256
PLAN_TILE = PLAN_IPT * PLAN_THREADS                    # 2048 rows per count block
PLAN_CARRY = 1024                                      # block sums per pass of the carry kernel
PLAN_CHUNK = 512
PLAN_DEGREES = (513, 1024, 1025, 1537)                 # 2, 2, 3, 4 chunks: the offsets are a multiple of nothing
PLAN_N_SMALL = 3 * PLAN_TILE + 5
# last row of thread 0 | first of thread 1; wave 0 | 1; into wave 3; block 0 | 1; block 1 | 2; the last row, in a block that is not full
PLAN_LONG_SMALL = (7, 8, 511, 512, 1535, 1536, 2047, 2048, 4095, 4096, PLAN_N_SMALL - 1)
PLAN_N_BIG = (PLAN_CARRY + 1) * PLAN_TILE + 3          # 1026 count blocks: the carry kernel takes a second pass
# block 0; the last row the first carry pass covers; the first row of the second pass; the last row
PLAN_LONG_BIG = (5, (PLAN_CARRY - 1) * PLAN_TILE + PLAN_TILE - 1, PLAN_CARRY * PLAN_TILE, PLAN_N_BIG - 1)
PLAN_BROKEN = ("no_cross_wave", "no_block_carry", "no_pass_base", "shifted")
PLAN_U = 2.0 ** -24
PLAN_STALE = np.frombuffer(b"\xa5\xa5\xa5\xa5", dtype=np.float32)[0]    # what a partial that nobody wrote holds in a 0xA5-filled workspace


def csr_plan_reference(deg, broken=None):
    """The planner's three launches in numpy on the clamped degrees of the n rows -> (chunks [n], off [n], total).
    chunks[r] = ceil(deg / 512) where deg > 512, else 0; off = the exclusive prefix sum of chunks; total = their sum (carry[nb]).
    Computed the way the kernels do -- 8 rows per thread, a shuffle scan over the 64 lanes, the sums of the waves before, the
    block's carry, the carry kernel's passes of 1024 block sums with a running base -- so that one step can be left out:
    broken = "no_cross_wave" (before += wave_sum[i] missing), "no_block_carry" (carry[r / kCountTile] not added),
    "no_pass_base" (base_sh += tile missing: every pass starts at 0 and carry[nb] is 0), "shifted" (every offset + total)."""
    assert broken is None or broken in PLAN_BROKEN
    deg = np.asarray(deg, dtype=np.int64)
    n = len(deg)
    chunks = np.where(deg > PLAN_CHUNK, -(-deg // PLAN_CHUNK), 0)
    nb = -(-n // PLAN_TILE)
    c = np.zeros(nb * PLAN_TILE, dtype=np.int64)
    c[:n] = chunks
    c = c.reshape(nb, PLAN_THREADS // PLAN_WAVE, PLAN_WAVE, PLAN_IPT)
    s = c.sum(3)                                                   # a thread's 8 rows
    lane_excl = np.cumsum(s, 2) - s                                # incl - s after the shuffles
    wave_sum = s.sum(2)
    before = np.cumsum(wave_sum, 1) - wave_sum
    if broken == "no_cross_wave":
        before[:] = 0
    local = before[:, :, None, None] + lane_excl[:, :, :, None] + (np.cumsum(c, 3) - c)
    block = wave_sum.sum(1)
    carry = np.zeros(nb + 1, dtype=np.int64)
    base = 0
    for t0 in range(0, nb, PLAN_CARRY):
        x = block[t0:t0 + PLAN_CARRY]
        carry[t0:t0 + len(x)] = base + np.cumsum(x) - x
        if broken != "no_pass_base":
            base += int(x.sum())
    carry[nb] = base
    off = local.reshape(-1)[:n].copy()
    if broken != "no_block_carry":
        off += carry[np.arange(n) // PLAN_TILE]
    total = int(carry[nb])
    if broken == "shifted":
        off += total
    return chunks, off, total


def csr_plan_case(n, long_rows, seed, filler=6):
    """A rectangular CSR of n rows over ids in [0, n) -> (rowptr int64 [n + 1], col int32, deg int64 [n]).  Row long_rows[i] has
    PLAN_DEGREES[i % 4] entries; the rows beside a long row that are not long themselves are empty; every other row has 0..filler.
    Ids are random; every second long row holds its own id -- as the last entry, or as the first entry of its last chunk."""
    rs = np.random.default_rng(seed)
    long_rows = np.asarray(long_rows, dtype=np.int64)
    deg = rs.integers(0, filler + 1, n).astype(np.int64)
    beside = np.concatenate([long_rows - 1, long_rows + 1])
    deg[beside[(beside >= 0) & (beside < n)]] = 0
    deg[long_rows] = np.asarray(PLAN_DEGREES)[np.arange(len(long_rows)) % len(PLAN_DEGREES)]
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=rowptr[1:])
    col = rs.integers(0, n, int(rowptr[-1])).astype(np.int32)
    for i, p in enumerate(long_rows):
        own = col[rowptr[p]:rowptr[p + 1]] == p
        col[rowptr[p]:rowptr[p + 1]][own] = (p + 2) % n               # no accidental self entry
        if i % 2 == 0:
            last_chunk = rowptr[p] + (deg[p] - 1) // PLAN_CHUNK * PLAN_CHUNK
            col[rowptr[p + 1] - 1 if i % 4 == 0 else last_chunk] = p
    return rowptr, col, deg


def csr_plan_perm(n, long_rows, seed):
    """A permutation of [0, n) without a fixed point among the long rows that maps long rows to long rows (rotated by one) and the
    others among themselves: as a node list it keeps the long rows at their positions while row != node id."""
    rs = np.random.default_rng(seed)
    long_rows = np.asarray(long_rows, dtype=np.int64)
    perm = np.empty(n, dtype=np.int64)
    rest = np.setdiff1d(np.arange(n), long_rows)
    perm[rest] = rs.permutation(rest)
    perm[long_rows] = np.roll(long_rows, 1)
    return perm


def plan_gamma(length, extra=0):
    """Higham's gamma_m (Accuracy and Stability of Numerical Algorithms, section 4.2) for a sum of `length` terms in 512-term chunks:
    m = min(length, 512) + ceil(length / 512) + extra -- the longest chain of additions is one chunk plus the chunk adds
    (tests/test_gpu_csr_sum.py's gamma_bound); extra = 2 for a mean (the self term, the multiplication by fl(1 / c)) and for a
    weighted term (the weight's rounding and the product's)."""
    length = np.asarray(length, dtype=np.float64)
    m = np.minimum(length, PLAN_CHUNK) + np.ceil(length / PLAN_CHUNK) + extra
    return m * PLAN_U / (1 - m * PLAN_U)


def csr_row_sums(rowptr, col, table):
    """fp64 (sums, sums of magnitudes) [n, dim] of the rows of a CSR whose ids are inside the table, by np.add.reduceat"""
    t = np.asarray(table)
    n = len(rowptr) - 1
    deg = np.diff(rowptr)
    ids = col[:int(rowptr[-1])]
    tot, mass = np.zeros((n, t.shape[1])), np.zeros((n, t.shape[1]))
    has = deg > 0
    starts = rowptr[:-1][has]                                         # strictly increasing: the empty rows own no entries
    for c0 in range(0, t.shape[1] if has.any() else 0, 128):          # 128 columns at a time: [E, dim] in fp64 is large at dim 1433
        rows = t[:, c0:c0 + 128].astype(np.float64)[ids]
        tot[has, c0:c0 + 128] = np.add.reduceat(rows, starts, axis=0)
        mass[has, c0:c0 + 128] = np.add.reduceat(np.abs(rows), starts, axis=0)
    return tot, mass


def csr_rows_reference(rowptr, col, table, nodes=None, self_loop=False, flag=False, mean=True, sums=None):
    """fp64 row sums (mean=False: sage_csr_sum) or means (sage_csr_mean) of the rows `nodes` (None: every row) of a CSR whose ids
    are inside the table, by np.add.reduceat -> (ref [rows, dim], bar [rows, dim], ceff [rows]).  The mean adds the node's own row
    where self_loop and the row does not hold it, and divides by the count; a set without a term is zeros (NaN with `flag`).
    bar = gamma_m * sum|terms| (/ count), m = plan_gamma's with 2 more for a mean.  Derived, not measured.
    sums: csr_row_sums of the same arguments, to share among calls (left unchanged)."""
    t = np.asarray(table)
    n = len(rowptr) - 1
    deg = np.diff(rowptr)
    tot, mass = (x.copy() for x in (csr_row_sums(rowptr, col, table) if sums is None else sums))
    extra = np.zeros(n, dtype=bool)
    if mean and self_loop:
        src = np.repeat(np.arange(n), deg)
        own = np.zeros(n, dtype=bool)
        own[src[col[:len(src)] == src]] = True
        extra = ~own
        tot[extra] += t[:n][extra].astype(np.float64)
        mass[extra] += np.abs(t[:n][extra].astype(np.float64))
    ceff = deg + extra
    if nodes is not None:
        nodes = np.asarray(nodes, dtype=np.int64)
        tot, mass, ceff, deg = tot[nodes], mass[nodes], ceff[nodes], deg[nodes]
    if not mean:
        return tot, plan_gamma(deg)[:, None] * mass, ceff
    d = np.maximum(ceff, 1)[:, None]
    ref = tot / d
    ref[ceff == 0] = np.nan if flag else 0.0
    return ref, plan_gamma(deg, 2)[:, None] * mass / d, ceff


def plan_miss(got, ref, bar, what=""):
    """How `got` misses a planner test's bar: None when it meets it, else a message.  NaNs must coincide, elements without a term
    (bar 0) are exact, every other element is within its bar.  Prints the largest err / bar (information only)."""
    got = np.asarray(got, dtype=np.float64)
    if got.shape != ref.shape:
        return f"{what}: shape {got.shape} vs {ref.shape}"
    if not np.array_equal(np.isnan(got), np.isnan(ref)):
        return f"{what}: NaN pattern differs in rows {np.nonzero((np.isnan(got) != np.isnan(ref)).any(1))[0][:8].tolist()}"
    fin = ~np.isnan(ref)
    err = np.where(fin, np.abs(np.where(fin, got - ref, 0.0)), 0.0)
    ratio = np.where(bar > 0, err / np.maximum(bar, 1e-300), np.where(err > 0, np.inf, 0.0))
    worst = float(ratio.max()) if ratio.size else 0.0
    print(f"{what}: max err / bound = {worst:.3f}")
    if worst > 1.0:
        r, c = np.unravel_index(np.argmax(ratio), ratio.shape)
        return f"{what}: row {r} column {c}: |got - ref| = {err[r, c]:.3e} > bar {bar[r, c]:.3e} ({int((ratio > 1).sum())} elements over)"
    return None


def csr_mean_under_plan(rowptr, col, table, rows, off, total, cap, self_loop, last_wins=True):
    """What sage_csr_mean's chunk and row kernels make of rows `rows` (row r = node r) given the plan (off, total = carry[nb]) and a
    workspace of `cap` items filled with 0xA5 bytes, in numpy fp32 with the kernels' order of additions -> {row: [dim] fp32}.
    csr_expand_kernel: a long row whose chunks fit writes its id into item_row[off .. off + k) (two rows that claim one item race:
    the later row wins, or the earlier one with last_wins=False); csr_chunk_kernel: item i < min(total, cap) is summed for the row
    item_row[i] names if that row's range holds i (chunk_item), every other partial stays stale; csr_row_kernel: a row that fits adds
    partials[off .. off + k) -- whoever wrote them -- and takes has_self from there, any other long row sums its chunks in place."""
    t = np.asarray(table, dtype=np.float32)
    deg = np.diff(rowptr)
    k_of = {int(r): int(-(-deg[r] // PLAN_CHUNK)) if deg[r] > PLAN_CHUNK else 0 for r in rows}
    fits = {r: k_of[r] > 0 and off[r] + k_of[r] <= cap for r in k_of}
    item_row = {}
    for r in (sorted(k_of) if last_wins else sorted(k_of, reverse=True)):
        if fits[r]:
            for i in range(int(off[r]), int(off[r]) + k_of[r]):
                item_row[i] = r

    def chunk(r, c):
        b = int(rowptr[r]) + c * PLAN_CHUNK
        e = min(b + PLAN_CHUNK, int(rowptr[r + 1]))
        ids = col[b:e]
        return np.cumsum(t[ids], axis=0, dtype=np.float32)[-1], bool((ids == r).any())      # sequential fp32, in stored order

    items = min(int(total), int(cap))
    partial, has_self = {}, {}
    for i, r in item_row.items():
        if i < items:
            partial[i], has_self[i] = chunk(r, i - int(off[r]))
    stale = np.full(t.shape[1], PLAN_STALE, dtype=np.float32)
    out = {}
    for r in k_of:
        s = np.zeros(t.shape[1], dtype=np.float32)
        found = False
        if fits[r]:
            for i in range(int(off[r]), int(off[r]) + k_of[r]):
                s = s + partial.get(i, stale)
                found |= has_self.get(i, True)                       # 0xA5A5A5A5 != 0
        elif k_of[r] > 0:
            for c in range(k_of[r]):
                p, f = chunk(r, c)
                s = s + p
                found |= f
        else:
            ids = col[rowptr[r]:rowptr[r + 1]]
            if len(ids):
                s = np.cumsum(t[ids], axis=0, dtype=np.float32)[-1]
            found = bool((ids == r).any())
        extra = bool(self_loop) and not found
        if extra:
            s = s + t[r]
        ceff = int(deg[r]) + int(extra)
        out[r] = (s * (np.float32(1.0) / np.float32(ceff))).astype(np.float32) if ceff else np.zeros_like(s)
    return out


def plan_item_cap(rows, max_edges):
    """chunk_ws's item capacity: max_edges / 512 + min(rows, max_edges / 513)"""
    return max_edges // PLAN_CHUNK + min(rows, max_edges // (PLAN_CHUNK + 1))


def plan_tight_max_edges(rows, total):
    """The smallest max_edges whose item list holds `total` items.  The list is then (almost always exactly) as long as the plan:
    a long row whose offset is too large by anything no longer fits and is summed by its row wave."""
    me = 0
    while plan_item_cap(rows, me) < total:
        me += 1
    return me


def embed_plan_case(embed_rows, long_rows, seed, n_sets=312, k=64):
    """Sampled sets (nbr int32 [n_sets, k], cnt int32 [n_sets]) whose terms give embedding row long_rows[i] exactly
    PLAN_DEGREES[i % 4] terms; the other terms name random other rows (runs of about one).  cnt cycles through k, k, k - 4, k, 0, k,
    33, k; padding is -1."""
    rs = np.random.default_rng(seed)
    long_rows = np.asarray(long_rows, dtype=np.int64)
    lens = np.asarray(PLAN_DEGREES)[np.arange(len(long_rows)) % len(PLAN_DEGREES)]
    cnt = np.asarray([k, k, k - 4, k, 0, k, 33, k])[np.arange(n_sets) % 8].astype(np.int32)
    terms = int(cnt.sum())
    assert terms > lens.sum()
    rest = np.setdiff1d(np.arange(min(embed_rows, 1 << 22)), long_rows)
    keys = np.concatenate([np.repeat(long_rows, lens), rs.choice(rest, terms - int(lens.sum()))])
    keys = keys[rs.permutation(terms)]
    nbr = np.full((n_sets, k), -1, dtype=np.int32)
    nbr[np.arange(k)[None, :] < cnt[:, None]] = keys                 # row-major: set t holds the next cnt[t] keys
    return nbr, cnt


def embed_plan_reference(grad, nbr, cnt, embed_rows, rows=None):
    """fp64 sums of grad[t] / c_t per embedding row by np.add.at -> (ref, bar) [embed_rows, dim] (rows given: the compact arrays
    over those ascending ids).  bar = gamma_m * sum|terms|, m = plan_gamma's of the row's term count with 2 more for the weight."""
    g = np.asarray(grad, dtype=np.float64)
    k = nbr.shape[1]
    c = np.minimum(cnt, k).astype(np.int64)
    held = np.arange(k)[None, :] < c[:, None]
    keys = nbr[held].astype(np.int64)
    sets = np.repeat(np.arange(len(c)), c)
    term = g[sets] / c[sets, None]
    if rows is not None:
        keys = np.searchsorted(rows, keys)
        embed_rows = len(rows)
    ref, mass = np.zeros((embed_rows, g.shape[1])), np.zeros((embed_rows, g.shape[1]))
    np.add.at(ref, keys, term)
    np.add.at(mass, keys, np.abs(term))
    return ref, plan_gamma(np.bincount(keys, minlength=embed_rows), 2)[:, None] * mass
