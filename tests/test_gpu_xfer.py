"""to_host / to_device (gvamp_amd/csrc/gv_xfer.hip) on the device, with the host copies shared among 0, 1 and 15 helper threads
(GV_XFER_THREADS; CopyPool, gvamp_amd/csrc/gv_copy_pool.h -- the header tests/test_host_threads_cpu.py runs under the sanitizers).
The pool reads the variable once, so every value gets a fresh child process, one after the other; the child holds the GPU alone and
starts nothing.  Whatever the number of helpers, the bytes must come back as they went:

  round trips         an M-space vector uploaded and downloaded at 32767, 32768, 32769 doubles (around the 256 KiB below which the caller
                      copies alone), 262145 (2 MiB, the piece of to_host, + 8 bytes), 1048576 and 1048577 (8 MiB, the staging buffer, and
                      8 bytes more) and 2621443 (two staging buffers and an odd rest)
  host pointers       gv_ax / gv_atx on host pointers against gv_ax_dev / gv_atx_dev on handles + download, bit for bit, on a shard of
                      8 individuals x 2621443 markers (N tiny: the data set stays a few MB, the M-space vector is the 21 MB one)
  shared pool         three threads, each with a context of its own, run the round trips at the same time through the one pool"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = [32767, 32768, 32769, 262145, 1048576, 1048577, 2621443]

CHILD = r"""
import json, sys, threading
sys.path.insert(0, %(root)r)
import numpy as np
from gvamp_amd import capi
LENS = %(lens)r
N, M = 8, 2621443

def same(a, b):
    return bool(a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)))

def round_trips(seed):
    # one context, resized from length to length; [[doubles, bytes came back equal], ...]
    out = []
    rng = np.random.default_rng(seed)
    with capi.Shard(N, LENS[0]) as rt:
        for n in LENS:
            rt.set_dims(N, n)
            a = rng.standard_normal(n)
            a[::1001] = -0.0
            v = rt.vecM(a)
            out.append([n, same(v.download(), a)])
            b = rng.standard_normal(n)                 # once more into the same vector: the staging buffer held a's bytes
            v.upload(b)
            out[-1][1] = out[-1][1] and same(v.download(), b)
            v.free()
    return out

res = {"round_trips": round_trips(1)}
with capi.Shard(N, M) as sh:
    sh.synth_bed(7, miss_ppm=5000)
    sh.compute_markers_statistics()
    rng = np.random.default_rng(2)
    x, p = rng.standard_normal(M), rng.standard_normal(4 * sh.mbytes)
    p[N:] = 0.0
    xd, zd, pd, wd = sh.vecM(x), sh.vecN(), sh.vecN(p), sh.vecM()
    sh.ax_dev(xd, zd)
    sh.atx_dev(pd, wd)
    z, w = zd.download(), wd.download()
    res["ax"] = same(sh.Ax(x), z) and bool(np.any(z != 0.0))
    res["atx"] = same(sh.ATx(p), w) and bool(np.any(w != 0.0))
    res["ax_again"] = same(sh.Ax(x), z)               # behind the 21 MB download of ATx
shared = [None] * 3
def work(t):
    try:
        shared[t] = round_trips(10 + t)
    except Exception as e:                            # (reported on the result line)
        shared[t] = repr(e)
th = [threading.Thread(target=work, args=(t,)) for t in range(3)]
for t in th:
    t.start()
for t in th:
    t.join()
res["shared"] = shared
print("XFER " + json.dumps(res))
"""


def test_vectors_cross_unchanged_with_0_1_and_15_copy_helpers():
    want = [[n, True] for n in LENS]
    for helpers in (0, 1, 15):
        env = dict(os.environ, GV_XFER_THREADS=str(helpers))
        res = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "lens": LENS}], env=env, capture_output=True, text=True, timeout=180)
        assert res.returncode == 0, (helpers, res.returncode, res.stderr[-2000:])        # (the first child that fails ends the test)
        lines = [ln for ln in res.stdout.splitlines() if ln.startswith("XFER ")]
        assert len(lines) == 1, (helpers, res.stdout[-2000:])
        got = json.loads(lines[0][5:])
        assert got["round_trips"] == want, (helpers, got["round_trips"])
        assert got["ax"] is True and got["atx"] is True and got["ax_again"] is True, (helpers, got)
        assert got["shared"] == [want, want, want], (helpers, got["shared"])
