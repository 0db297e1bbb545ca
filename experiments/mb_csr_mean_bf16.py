"""The bf16 feature table (sage_csr_mean_bf16) against the fp32 one at configs[2]'s size, in ONE process, the forms alternating.

One JSON line per case.  Graph: rmat_graph(20, 16_000_000, seed=0), bench.py's configs[2] graph.  The table is rounded to bf16 once;
the fp32 side reads its exact widening, so both sides compute the same bits (checked here at the sizes timed).  Times: device events
around the call, after warm-up; every repetition runs each form once, in turn, so that a drift of the box hits all of them; median,
min and max of --reps.  "fp32" appears twice (fp32, fp32_again): the distance between the two is the spread a difference has to beat.
  csr_mean     all rows, widths --dims (default 256 and 100, both on the vector path; an odd width takes the scalar one): the library's
               bf16 form, and every --variant
  embed_nodes  4096 seeds through inference.embed_nodes, gcn and concat
  exact_step   one ExactBatchTrainer.step for 4096 seeds, gcn and concat
  memory       peak allocated above the table during embed_all_nodes and during one exact step, and the table's own bytes
--variant LABEL=IN_FLIGHT,COLS builds csrc/sage_csr_mean.hip with -DSAGE_CSR_BF16_IN_FLIGHT / -DSAGE_CSR_BF16_COLS into --variant-dir
(if it is not there yet; --build-only stops after that, and needs no GPU) and times its sage_csr_mean_bf16 beside the library's.
Run on an MI355X: python experiments/mb_csr_mean_bf16.py --variant r8c4=8,4 --variant r16c4=16,4 --variant r16c8=16,8
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "graphsage-simple_amd")]
CSRC = os.path.join(REPO, "graphsage-simple_amd", "csrc")

from sage355 import native, ops  # noqa: E402


def build_variant(path, in_flight, cols):
    if os.path.exists(path):
        return
    os.makedirs(os.path.dirname(path), exist_ok=True)
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", f"-I{os.path.join(REPO, 'include')}", f"-I{CSRC}",
           "-Wno-unused-function", f"-DSAGE_CSR_BF16_IN_FLIGHT={in_flight}", f"-DSAGE_CSR_BF16_COLS={cols}", "-shared",
           os.path.join(CSRC, "sage_csr_mean.hip"), os.path.join(CSRC, "sage_api.hip"), "-o", path]
    subprocess.run(cmd, check=True)


def variant_call(path):
    """csr_mean over a bf16 table through the sage_csr_mean_bf16 of another build of the kernel file."""
    L = ctypes.CDLL(path)
    L.sage_csr_mean_bf16.argtypes = native.lib().sage_csr_mean.argtypes
    L.sage_csr_mean_bf16.restype = ctypes.c_int32
    L.sage_last_error.restype = ctypes.c_char_p

    def call(rp, cl, table, flag, out, ws):
        n, dim = out.shape
        rc = L.sage_csr_mean_bf16(native.ptr(rp), native.ptr(cl), n, None, n, cl.numel(), native.ptr(table), table.shape[0], table.stride(0), dim, 0,
                                  native.ptr(flag), native.ptr(out), out.stride(0), native.ptr(ws), ws.numel(), native.stream_handle())
        if rc != 0:
            raise RuntimeError(L.sage_last_error())
    return call


def timed_in_turn(forms, warmup, reps):
    """forms: {label: callable}.  -> {label: (median, min, max)} in seconds; every repetition runs each form once, in turn."""
    for _ in range(warmup):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in forms}
    for _ in range(reps):
        for k, fn in forms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b) * 1e-3)
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in ts.items()}


def report(case, res, **more):
    base = res["fp32"][0]
    for k, (med, lo, hi) in res.items():
        print(json.dumps(dict(case=case, form=k, ms=round(med * 1e3, 3), ms_min=round(lo * 1e3, 3), ms_max=round(hi * 1e3, 3),
                              vs_fp32=round(med / base, 3), **more)), flush=True)


def bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def peak_above(fn):
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edges", type=int, default=16_000_000)
    ap.add_argument("--dims", type=int, nargs="+", default=[256, 100])
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--seeds", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--variant", action="append", default=[], help="LABEL=IN_FLIGHT,COLS")
    ap.add_argument("--variant-dir", default=os.path.join(REPO, "build", "csr_mean_bf16_variants"))
    ap.add_argument("--build-only", action="store_true")
    args = ap.parse_args()
    variants = {}
    for v in args.variant:
        label, spec = v.split("=")
        in_flight, cols = (int(x) for x in spec.split(","))
        variants[label] = os.path.join(args.variant_dir, f"libcsr_mean_bf16_r{in_flight}_c{cols}.so")
        build_variant(variants[label], in_flight, cols)
    if args.build_only:
        return
    if not torch.cuda.is_available():
        raise SystemExit("mb_csr_mean_bf16 needs an MI355X")
    from sage355.exactbatch import ExactBatchTrainer
    from sage355.graph import rmat_graph
    from sage355.inference import _nonempty_flag, embed_all_nodes, embed_nodes

    g = rmat_graph(args.scale, args.edges, seed=0)
    n, nnz, h = g.num_nodes, g.nnz, args.hidden
    rp, cl = g.to("cuda")
    flag = _nonempty_flag(rp)
    box = torch.cuda.get_device_name(0)
    print(json.dumps(dict(case="setup", box=box, graph=f"rmat({args.scale}, {args.edges})", nodes=n, nnz=nnz, reps=args.reps, warmup=args.warmup)),
          flush=True)
    calls = {k: variant_call(p) for k, p in variants.items()}

    for dim in args.dims:
        t16 = torch.randn(n, dim, generator=torch.Generator().manual_seed(0)).cuda().to(torch.bfloat16)
        t32 = t16.float()
        ws = torch.empty(ops.csr_mean_workspace_bytes(n, nnz, dim), dtype=torch.uint8, device="cuda")
        outs = {k: torch.empty(n, dim, device="cuda") for k in ("fp32", "bf16", *calls)}
        forms = {"fp32": lambda: ops.csr_mean(rp, cl, t32, any_nonempty=flag, out=outs["fp32"], workspace=ws),
                 "bf16": lambda: ops.csr_mean(rp, cl, t16, any_nonempty=flag, out=outs["bf16"], workspace=ws)}
        for k, call in calls.items():
            forms[k] = (lambda call=call, k=k: call(rp, cl, t16, flag, outs[k], ws))
        forms["fp32_again"] = forms["fp32"]
        res = timed_in_turn(forms, args.warmup, args.reps)
        same = {k: bits_equal(outs[k], outs["fp32"]) for k in outs}
        report("csr_mean", res, dim=dim, table_MB_fp32=round(t32.numel() * 4 / 1e6, 1), table_MB_bf16=round(t16.numel() * 2 / 1e6, 1))
        print(json.dumps(dict(case="csr_mean_bits", dim=dim, equal_to_fp32=same)), flush=True)
        del t16, t32, ws, outs, forms
        torch.cuda.empty_cache()

    d0 = args.dims[0]
    t16 = torch.randn(n, d0, generator=torch.Generator().manual_seed(0)).cuda().to(torch.bfloat16)
    t32 = t16.float()
    deg = g.degrees()
    seeds_np = np.random.default_rng(0).choice(np.nonzero(deg > 0)[0], args.seeds, replace=False)
    seeds = torch.from_numpy(seeds_np.astype(np.int32)).cuda()
    labels = torch.from_numpy(np.random.default_rng(1).integers(0, 16, args.seeds)).cuda()
    gen = torch.Generator().manual_seed(1)
    for concat in (False, True):
        m = 2 if concat else 1
        enc = "concat" if concat else "gcn"
        w1 = (torch.randn(h, m * d0, generator=gen) / (m * d0) ** 0.5).cuda()
        w2 = (torch.randn(h, m * h, generator=gen) / (m * h) ** 0.5).cuda()
        fr = ops.CsrFrontier(n, "cuda", max_nodes=0)
        o = {}
        forms = {"fp32": lambda: o.__setitem__("fp32", embed_nodes(rp, cl, t32, w1, w2, seeds, concat=concat, frontier=fr)),
                 "bf16": lambda: o.__setitem__("bf16", embed_nodes(rp, cl, t16, w1, w2, seeds, concat=concat, frontier=fr))}
        forms["fp32_again"] = forms["fp32"]
        res = timed_in_turn(forms, args.warmup, args.reps)
        report("embed_nodes", res, encoder=enc, seeds=args.seeds, d0=d0, bits_equal=bits_equal(o["fp32"], o["bf16"]))
        trainers = {}
        for k, tab in (("fp32", t32), ("bf16", t16)):
            torch.manual_seed(7)
            trainers[k] = ExactBatchTrainer(rp, cl, tab, 16, hidden1=h, hidden2=h, gcn=not concat, lr=0.0)      # lr 0: every step is the same work
        loss = {}
        forms = {"fp32": lambda: loss.__setitem__("fp32", trainers["fp32"].step(seeds, labels)),
                 "bf16": lambda: loss.__setitem__("bf16", trainers["bf16"].step(seeds, labels))}
        forms["fp32_again"] = forms["fp32"]
        res = timed_in_turn(forms, args.warmup, args.reps)
        report("exact_step", res, encoder=enc, seeds=args.seeds, d0=d0, loss_bits_equal=bits_equal(loss["fp32"].reshape(1), loss["bf16"].reshape(1)))
        mem = {k: dict(table_bytes=tab.numel() * tab.element_size(),
                       embed_all_nodes_peak_above=peak_above(lambda: embed_all_nodes(rp, cl, tab, w1, w2, concat=concat)),
                       exact_step_peak_above=peak_above(lambda: trainers[k].step(seeds, labels)))
               for k, tab in (("fp32", t32), ("bf16", t16))}
        print(json.dumps(dict(case="memory", encoder=enc, nodes=n, d0=d0, **mem)), flush=True)
        del trainers, fr
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
