"""layer_tile16_kernel<KP, false, 13, 16> (csrc/sage_fused.hip): the layer-2 form the forward uses beside the one-launch layer 1 --
1024-thread blocks, one row per wave, 13 row loads of a lane group in flight -- against the fp64 oracle at its edge shapes.  Through
sage_layer_forward the form is reached with SAGE_T16_WAVES=16 SAGE_T16_INFLIGHT=13, which are read once per process: the checks run in
ONE child process.  Cases, oracle and tolerance (1e-5 of the pre-activation row maximum, NaN patterns equal) are those of
tests/test_gpu_layer_forward.py.

Shapes: rows 1, 15, 16, 17, 33 (partial tiles, a third tile); k 1, 13, 14, 25, 64 (KP = 128 fetches 2 ids per wave-instruction: 13 in
flight = 26 per trip, so 25 is one trip and 64 three; KP = 64 fetches 4: 52 per trip; 64 ids are one full wave-instruction of ids);
a row with count 0 alone and inside a mixed batch, with the flag that makes it NaN and without; dim 32 and 128, out_dim 16 and 128.
"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def alone_form_checks():
    import test_gpu_layer_forward as t
    worst = 0.0
    for dim in (32, 128):
        for out_dim in (16, 128):
            for n in (1, 15, 16, 17, 33):
                for k in (1, 13, 14, 25, 64):
                    c = t.Case(dim, n, k, out_dim, False, seed=1000 * dim + 10 * n + k, self_rows=(n + k) % 2 == 1, empty=0.15)
                    if n >= 15:
                        c.cnt[n // 2] = 0                      # a count-0 row inside a mixed batch, whatever the draw gave
                        if c.self_eff is not None:
                            c.self_eff[n // 2] = -1
                            c.self_row[n // 2] = -1
                        c.cnt_d[n // 2] = 0
                    for flag in (1, 0):
                        want, pre = c.oracle("relu", flag)
                        worst = max(worst, c.check(c.run("relu", flag=flag), want, pre, what=f"16 waves x 13 in flight, flag={flag}"))
            # a row with count 0 alone
            c = t.Case(dim, 1, 25, out_dim, False, seed=7 + dim + out_dim)
            c.cnt[:] = 0
            c.cnt_d.zero_()
            for flag in (1, 0):
                want, pre = c.oracle("relu", flag)
                assert bool(want.isnan().all()) == (flag == 1)
                c.check(c.run("relu", flag=flag), want, pre, what=f"one empty row, flag={flag}")
    return worst


_CHILD = r"""
import sys
sys.path[:0] = [{repo!r}, {repo!r} + "/graphsage-simple_amd", {repo!r} + "/tests"]
import test_gpu_layer2_alone_forms as t
print("worst |gpu - fp64| / rowmax = %.3e" % t.alone_form_checks())
print("ALONE_FORMS_OK")
"""


def test_one_trip_16_wave_form_matches_fp64(tmp_path):
    script = tmp_path / "alone_forms.py"
    script.write_text(_CHILD.format(repo=REPO))
    env = dict(os.environ, SAGE_T16_WAVES="16", SAGE_T16_INFLIGHT="13")
    res = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=300)
    print(res.stdout[-2000:])
    assert res.returncode == 0 and "ALONE_FORMS_OK" in res.stdout, res.stdout[-2000:] + res.stderr[-3000:]
