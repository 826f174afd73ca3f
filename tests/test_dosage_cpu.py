"""Compact dense data (8- / 16-bit dosage codes), the parts that need no GPU: the host reproducer of gv_synth_dosage, the new
C-ABI names, and the real-data driver's check of --geno-format (it must fail before any device work)."""
import os
import re
import subprocess

import numpy as np
import pytest

from gvamp_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ("gv_upload_dosage", "gv_upload_dosage_file", "gv_synth_dosage")


@pytest.mark.parametrize("bits", [8, 16])
def test_synth_dosage_is_deterministic_and_fills_the_code_range(bits):
    a = synth.synth_dosage(1500, 40, seed=5, bits=bits)
    assert a.shape == (40, 1500) and a.dtype == (np.uint8 if bits == 8 else np.uint16)
    assert np.array_equal(a, synth.synth_dosage(1500, 40, seed=5, bits=bits))
    assert not np.array_equal(a, synth.synth_dosage(1500, 40, seed=6, bits=bits))
    top = 1 << (bits - 1)
    assert np.any(a >= top)                   # a sign-extension bug in a kernel would show: the top half of the range occurs
    assert int(a.max()) > (3 << (bits - 2)) and int(a.min()) == 0
    # genotype g in {0, 1, 2} is code // (3 * 2^(bits-3)) clipped at 2; allele frequencies spread over about 0.01 - 0.5
    g = np.minimum(a // (3 << (bits - 3)), 2)
    jit = a.astype(np.int64) - g.astype(np.int64) * (3 << (bits - 3))
    assert np.all((jit >= 0) & (jit < (1 << (bits - 2))))
    freq = synth.synth_dosage(4000, 300, seed=9, bits=bits)
    f = np.minimum(freq // (3 << (bits - 3)), 2).mean(axis=1) / 2
    assert f.min() < 0.05 and f.max() > 0.4 and f.max() < 0.56


def test_the_two_widths_share_genotypes():
    """same seed: the genotype part of the 8- and the 16-bit codes is the same draw"""
    a8, a16 = synth.synth_dosage(300, 20, 3, 8), synth.synth_dosage(300, 20, 3, 16)
    assert np.array_equal(np.minimum(a8 // 96, 2), np.minimum(a16 // 24576, 2))


@pytest.mark.parametrize("bits", [8, 16])
def test_synth_dosage_offset_slice_equals_generation_at_S(bits):
    full = synth.synth_dosage(13, 40, seed=77, bits=bits)
    for S, M in ((0, 40), (7, 20), (39, 1)):
        assert np.array_equal(synth.synth_dosage(13, M, seed=77, bits=bits, S=S), full[S:S + M])


def test_synth_dosage_refuses_other_widths():
    with pytest.raises(ValueError):
        synth.synth_dosage(4, 4, 1, 12)


def test_new_abi_names_are_declared_and_exported():
    with open(os.path.join(ROOT, "include", "gvamp.h")) as f:
        hdr = f.read()
    for name in NEW_NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in capi.EXPORTS
    assert re.search(r"#define\s+GV_ABI_VERSION\s+4\b", hdr)          # additions only
    lib = os.path.join(ROOT, "gvamp_amd", "libgvamp.so")
    assert os.path.exists(lib), "libgvamp.so is built by build()"
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
    for name in NEW_NAMES:
        assert re.search(r"\bT %s$" % name, syms, re.M), name


def test_gvamp_main_real_rejects_unknown_geno_format_before_device_work(tmp_path):
    exe = os.path.join(ROOT, "gvamp_amd", "gvamp_main_real")
    assert os.path.exists(exe), "gvamp_main_real is built by build() (gvamp_amd/csrc/host/Makefile)"
    out = tmp_path / "out"
    r = subprocess.run([exe, "--run-mode", "infere", "--geno-format", "nope", "--bed-file", str(tmp_path / "codes.bin"),
                        "--N", "10", "--Mt", "10", "--out-dir", str(out)], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "--geno-format" in r.stdout + r.stderr and "nope" in r.stdout + r.stderr
    assert not os.path.exists(out)            # the parser stopped at the flag: nothing after it was acted on
    for a in ("0", "-1", "abc"):
        r = subprocess.run([exe, "--dosage-scale", a], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "--dosage-scale" in r.stdout + r.stderr
