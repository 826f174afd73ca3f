"""Methylation data, the parts that need no GPU: the host reproducer of gv_synth_meth, the new C-ABI names, and the
gvamp_sim_meth driver's option check (it must fail before any device work)."""
import os
import re
import subprocess

import numpy as np

from gvamp_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ("gv_upload_meth", "gv_upload_meth_file", "gv_synth_meth")


def test_synth_meth_is_deterministic_and_exactly_dyadic():
    a = synth.synth_meth(37, 11, seed=5)
    b = synth.synth_meth(37, 11, seed=5)
    assert a.shape == (11, 37) and a.dtype == np.float64
    assert np.array_equal(a, b)
    assert not np.array_equal(a, synth.synth_meth(37, 11, seed=6))
    # every value is k * 2^-19 with k < 2^19: exact in fp64 whatever the order of the arithmetic
    k = a * 2.0 ** 19
    assert np.array_equal(k, np.round(k)) and np.all(k >= 0) and np.all(k < 2 ** 19)
    assert np.all((a >= 0.0) & (a < 1.0))
    # the centre is per marker, the Irwin-Hall spread per entry
    assert np.ptp(a.mean(axis=1)) > 0.05 and np.all(a.std(axis=1) > 0.02)


def test_synth_meth_offset_slice_equals_generation_at_S():
    full = synth.synth_meth(13, 40, seed=77)
    for S, M in ((0, 40), (7, 20), (39, 1)):
        assert np.array_equal(synth.synth_meth(13, M, seed=77, S=S), full[S:S + M])


def test_new_abi_names_are_declared_and_exported():
    with open(os.path.join(ROOT, "include", "gvamp.h")) as f:
        hdr = f.read()
    for name in NEW_NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in capi.EXPORTS
    assert re.search(r"#define\s+GV_ABI_VERSION\s+4\b", hdr)
    lib = os.path.join(ROOT, "gvamp_amd", "libgvamp.so")
    if os.path.exists(lib):
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
        for name in NEW_NAMES:
            assert re.search(r"\bT %s$" % name, syms, re.M), name


def test_gvamp_sim_meth_rejects_unknown_flag_before_device_work(tmp_path):
    exe = os.path.join(ROOT, "gvamp_amd", "gvamp_sim_meth")
    assert os.path.exists(exe), "gvamp_sim_meth is built by build() (gvamp_amd/csrc/host/Makefile)"
    r = subprocess.run([exe, "--no-such-flag", "1", "--N", "10", "--Mt", "10", "--bed-file", str(tmp_path / "m.bin")],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "no-such-flag" in r.stdout + r.stderr
    assert not os.path.exists(tmp_path / "m.bin")        # nothing was simulated or written
