"""Layer 2's block shape follows the form of layer 1 (csrc/sage_fused.hip, launch_tile16): 1024-thread blocks with the whole neighbour
list in one trip when the forward's layer 1 is the one-launch phase-sliced kernel, 512-thread blocks and two trips otherwise,
SAGE_T16_WAVES / SAGE_T16_INFLIGHT overriding both.  The shape must never reach the bits: the same model's single forwards and its role
pipeline are compared bit for bit between the default (this process, variables unset) and child processes with every other combination
(the variables are read once per process), and the default is held against the fp64 oracle with smoke()'s bound.  Both forms of layer 1 are covered: the one-launch form (the default's 1024-thread layer 2)
and, with keep_means, gather + contraction (the default's 512-thread layer 2).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_MODEL = r"""
import sys
import numpy as np, torch
from sage355.engine import TwoHopEngine, RolePipeline
from sage355.graph import rmat_graph

g = rmat_graph(12, 60_000, seed=1)
gen = torch.Generator().manual_seed(0)
d0, h1, h2, k1, k2, b, depth = 256, 128, 128, 15, 25, 512, 2
table = torch.randn(g.num_nodes, d0, generator=gen).cuda()
w1 = (torch.randn(h1, d0, generator=gen) / 16).cuda()
w2 = (torch.randn(h2, h1, generator=gen) / 11).cuda()
seeds = np.random.default_rng(0).choice(np.nonzero(g.degrees() > 0)[0], b, replace=False).astype(np.int32)
n = 2 * depth + 1
sd = torch.from_numpy(np.stack([np.roll(seeds, 3 * i) for i in range(n)])).cuda()
rowptr, col = g.to("cuda")


def outputs():
    # -> [2 + n, b, h2]: a single forward with the one-launch layer 1, the same with gather + contraction (keep_means), n pipelined batches
    with torch.no_grad():
        eng = TwoHopEngine(rowptr, col, table, w1, w2, k1, k2, max_batch=b)
        assert eng.layout.layer1_split
        one = eng.forward(sd[0], seed=42).clone()
        assert eng.intermediates()["agg1"] is None, "the one-launch layer 1 did not run"
        eng.keep_means = True
        two = eng.forward(sd[0], seed=42).clone()
        assert eng.intermediates()["agg1"] is not None, "keep_means did not select gather + contraction"
        pipe = RolePipeline(rowptr, col, table, w1, w2, k1, k2, batch=b, depth=depth, threads=True)
        po = torch.empty(n, b, h2, device="cuda")
        pipe.submit_many(sd, [42 + i for i in range(n)], po)
        pipe.synchronize()
        return torch.cat([one[None], two[None], po]).cpu(), eng
"""

_CHILD = _MODEL + r"""
out, _ = outputs()
np.save(sys.argv[1], out.numpy())
print("CHILD OK")
"""

_default = {}


def default_outputs():
    if not _default:
        assert "SAGE_T16_WAVES" not in os.environ and "SAGE_T16_INFLIGHT" not in os.environ, "this test needs the library's own choice of layer 2's block shape"
        ns = {}
        exec(_MODEL, ns)
        _default["out"], _default["eng"], _default["ns"] = *ns["outputs"](), ns
    return _default


def test_default_forms_agree_and_match_fp64():
    from oracle import ref_sparse
    d = default_outputs()
    out, eng, ns = d["out"], d["eng"], d["ns"]
    assert torch.equal(out[0].view(torch.int32), out[1].view(torch.int32)), "the two forms of layer 1 (and of layer 2's block) differ"
    assert torch.equal(out[2].view(torch.int32), out[0].view(torch.int32)), "role pipeline differs from the single forward"
    with torch.no_grad():
        eng.keep_means = False
        got = eng.forward(ns["sd"][0], seed=42).cpu()
    it = eng.intermediates()
    first = it["first_frontier_row"]
    s1, nbr1, cnt1 = it["s1_nodes"].cpu().numpy(), it["nbr1"].cpu().numpy(), it["cnt1"].cpu().numpy()
    seeds_int = ns["seeds"] if eng._new_of_old is None else eng._new_of_old[torch.from_numpy(ns["seeds"]).long().cuda()].cpu().numpy()
    ref = ref_sparse.two_hop_forward(eng.table.cpu(), ns["w1"].cpu(), ns["w2"].cpu(), seeds_int, it["nbr2"].cpu().numpy(),
                                     it["cnt2"].cpu().numpy(), s1[first:], nbr1[first:], cnt1[first:], gcn=True)
    err = ((got.double() - ref).abs() / ref.abs().amax(1, keepdim=True).clamp_min(1e-30)).max().item()
    print(f"max |gpu - fp64| / rowmax = {err:.3e}")
    assert torch.equal(got.view(torch.int32), out[0].view(torch.int32))
    assert err <= 1e-5


@pytest.mark.parametrize("waves,inflight", [("8", "7"), ("16", "7"), ("16", "13")])
def test_block_shape_does_not_reach_the_bits(waves, inflight, tmp_path):
    want = default_outputs()["out"]
    script, dump = tmp_path / "child.py", tmp_path / "out.npy"
    script.write_text(_CHILD)
    env = dict(os.environ, SAGE_T16_WAVES=waves, SAGE_T16_INFLIGHT=inflight,
               PYTHONPATH=os.pathsep.join([REPO, os.path.join(REPO, "graphsage-simple_amd"), os.environ.get("PYTHONPATH", "")]))
    res = subprocess.run([sys.executable, str(script), str(dump)], env=env, capture_output=True, text=True, timeout=300)
    print(res.stdout[-2000:], res.stderr[-2000:])
    assert res.returncode == 0 and "CHILD OK" in res.stdout
    got = torch.from_numpy(np.load(dump))
    assert got.shape == want.shape
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), f"SAGE_T16_WAVES={waves} SAGE_T16_INFLIGHT={inflight} changes the forward's bits"
