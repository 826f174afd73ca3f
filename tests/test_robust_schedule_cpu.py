"""--model robust's delta_H schedule and guard on the CPU: the restatement of the product's loop against the
reference-order restatement, the small-N case both ways, and the driver's refusal of an unknown schedule."""
import os
import re
import subprocess

import numpy as np
import pytest

from gvamp_amd import hostapi

import robust_restatement as rr
import robust_schedule_restatement as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_schedule_is_robust_run_bit_for_bit():
    D = rs.case(3000, 300, 8, 9)[1]
    y = rs.case(3000, 300, 8, 9)[3]
    kw = dict(iterations=5, gam1=1e-8, rho=0.5, CG_max_iter=30, seed=4, stop_criteria_thr=1e-12)
    a = rr.robust_run(D, y, [0.7, 0.3], [0.0, 0.09], **kw)
    b = rs.robust_run(D, y, [0.7, 0.3], [0.0, 0.09], schedule="reference", **kw)
    assert b.stopped is None and len(a) == len(b) == 5
    for p, q in zip(a, b):
        for k in p:
            assert np.array_equal(p[k], q[k]), k
    assert [q["deltaH_applied"] for q in b] == [1e-3] + [p["deltaH"] for p in a[:-1]]


@pytest.mark.parametrize("noise", ["gaussian", "contaminated"])
def test_small_n_deferred_converges_where_the_reference_order_breaks_down(noise):
    """the 300 x 60 case of test_robust_cpu.py: the deferred step picks delta_H on the cavity it is applied to, so some residuals
    fall inside iteration 2's threshold; in the reference's order none does and the guard stops the run in iteration 2"""
    _bed, D, beta, y = rs.case(300, 60, 8, 9, noise)
    kw = dict(iterations=8, gam1=1e-8, rho=0.5, CG_max_iter=30, seed=4, stop_criteria_thr=1e-12)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = rs.robust_run(D, y, [0.7, 0.3], [0.0, 0.09], **kw)
        ref = rs.robust_run(D, y, [0.7, 0.3], [0.0, 0.09], schedule="reference", **kw)
    assert out.stopped is None and len(out) == 8
    assert out[0]["deltaH_applied"] == 1e-3 and out[0]["deltaH"] == 1e-3          # iteration 1 takes no step
    assert max(t["beta1"] for t in out[1:]) < 0.99
    assert np.corrcoef(out[-1]["x1"], beta)[0, 1] > 0.9
    it, delta, tau1, beta1 = ref.stopped
    assert (it, beta1, len(ref)) == (2, 1.0, 1) and delta <= 1e-3 and tau1 > 1e-3


def test_unknown_schedule_is_refused_by_the_driver():
    exe = os.path.join(ROOT, "gvamp_amd", "gvamp_main_real")
    if not os.path.exists(exe):
        pytest.skip("gvamp_main_real is not built")
    r = subprocess.run([exe, "--model", "robust", "--huber-delta-schedule", "early"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "--huber-delta-schedule has to be deferred or reference" in r.stdout and "early" in r.stdout


def test_host_abi_mirrors_the_header():
    with open(os.path.join(ROOT, "include", "gvamp_host.h")) as f:
        hdr = f.read()
    assert int(re.search(r"#define\s+GVH_ABI_VERSION\s+(\d+)", hdr).group(1)) == hostapi.HOST_ABI_VERSION
    opts = re.search(r"typedef struct \{(.*?)\} gvh_opts;", hdr, re.S).group(1)
    assert re.search(r"const char\* model;", opts) and re.search(r"const char\* huber_delta_schedule;", opts)
    assert [f for f, _ in hostapi.Opts._fields_][-2:] == ["model", "huber_delta_schedule"]
    assert [f for f, _ in hostapi.Iter._fields_][-1] == "deltaH"
