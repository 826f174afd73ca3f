"""Missing entries in compact dosage data (gv_set_dosage_missing), the parts that need no GPU: the restatement of the contract
(tests/dosage_na_restatement.py) pinned to the bed path's semantics, the host twin of gv_synth_dosage_na, and the new C-ABI names."""
import os
import re
import subprocess

import numpy as np
import pytest

import dosage_na_restatement as dr
import precond_restatement as pr
from gvamp_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
DTYPE = {8: np.uint8, 16: np.uint16}
STEP = {8: 64, 16: 16384}                       # hard calls as codes: 64 {0, 1, 2} at scale 2^-6, 16384 {0, 1, 2} at 2^-14
DYADIC = {8: 2.0 ** -6, 16: 2.0 ** -14}
NEW_NAMES = ("gv_set_dosage_missing", "gv_synth_dosage_na", "gv_dosage_info", "gv_marker_counts")


def close(a, b, tol=1e-13):
    """|a - b| <= tol (|b| + max |b|): relative, with the largest magnitude as the floor for entries that cancel to near zero"""
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    return bool(np.all(np.abs(a - b) <= LD(tol) * (np.abs(b) + np.max(np.abs(b)))))


def bed_as_codes(bed, N, M, bits):
    a, b = pr.decode(bed, N, M)                             # N x M: hard calls (0 at missing) and presence
    B = (a.T * STEP[bits]).astype(DTYPE[bits])
    B[b.T == 0] = dr.reserved(bits)
    return a, b, B


@pytest.mark.parametrize("with_na", [False, True])
@pytest.mark.parametrize("bits", [8, 16])
def test_restatement_equals_the_bed_path_on_codes_of_a_bed_with_missing_genotypes(bits, with_na):
    N, M = 403, 60
    bed = synth.synth_bed(N, M, seed=12, miss_ppm=20000)
    a, b, B = bed_as_codes(bed, N, M, bits)
    assert (b == 0).sum() > 100 and np.any(B == dr.reserved(bits))
    na = np.ones(N)
    if with_na:
        na[3::7] = 0.0
    mave, msig = pr.marker_stats(a, b, na)
    st = dr.stats(B, bits, na, DYADIC[bits])
    assert np.array_equal(st["cnt"], (b * na[:, None]).sum(0).astype(np.int64))
    assert close(st["mave"], mave) and close(st["msig"], msig)
    # the bed operator carries the phenotype mask, the dense one does not (gv_ax applies none): equal at the individuals with a phenotype
    A_bed, A = pr.matrix(a, b, na, mave, msig), dr.matrix(st)
    assert close(A * na.astype(LD)[:, None], A_bed)
    if with_na:
        assert np.all(A_bed[na == 0] == 0) and np.any(A[na == 0] != 0)
    assert np.all(A[b == 0] == 0)                           # a missing entry is an exact zero of the operator


@pytest.mark.parametrize("bits", [8, 16])
def test_without_a_reserved_code_the_restatement_is_the_existing_dosage_definition(bits):
    N, M = 211, 40
    B = synth.synth_dosage_na(N, M, 3, bits, 0)
    assert not np.any(B == dr.reserved(bits))
    B[0] = 200 if bits == 8 else 40001                      # a constant row
    na = np.ones(N)
    na[3::7] = 0.0
    nonas = int(na.sum())
    scale = 1.0 / 127.0 if bits == 8 else 2.0 ** -14
    for alpha in (1.0, 0.3):
        on, off = dr.stats(B, bits, na, scale, alpha), dr.stats(B, bits, na, scale, alpha, missing=False)
        # the definition of include/gvamp.h without missing entries (tests/test_gpu_dosage.py: ref_code_stats / ref_stats)
        s = (B.astype(np.int64) * na.astype(np.int64)[None, :]).sum(axis=1)
        mu = s.astype(LD) / LD(nonas)
        D = B.astype(LD) - mu[:, None]
        q = ((D * D) * na.astype(LD)[None, :]).sum(axis=1)
        msig = np.where(q != 0, (LD(scale) * np.sqrt(np.where(q != 0, q, LD(1)) / LD(nonas - 1))) ** LD(-alpha), LD(1))
        for st in (on, off):
            assert np.all(st["cnt"] == nonas)
            assert np.array_equal(st["mu"], mu) and np.array_equal(st["q"], q) and np.array_equal(st["msig"], msig)
            assert np.array_equal(st["D"], D) and st["msig"][0] == 1
    # with the option off the reserved code is the value it is
    B[1, 5] = dr.reserved(bits)
    off = dr.stats(B, bits, na, scale, missing=False)
    assert off["cnt"][1] == nonas and off["D"][1, 5] == LD(dr.reserved(bits)) - off["mu"][1]
    assert dr.stats(B, bits, na, scale)["cnt"][1] == nonas - 1


@pytest.mark.parametrize("bits", [8, 16])
def test_synth_dosage_na_is_deterministic_sliceable_and_keeps_the_reserved_code_for_missing(bits):
    N, M, ppm = 1500, 40, 30000
    R = dr.reserved(bits)
    a = synth.synth_dosage_na(N, M, 5, bits, ppm)
    assert a.shape == (M, N) and a.dtype == DTYPE[bits]
    assert np.array_equal(a, synth.synth_dosage_na(N, M, 5, bits, ppm))
    assert not np.array_equal(a, synth.synth_dosage_na(N, M, 6, bits, ppm))
    for S, Ms in ((0, 40), (7, 20), (39, 1)):               # a shard [S, S + M) equals the rows of the whole matrix
        assert np.array_equal(synth.synth_dosage_na(N, Ms, 5, bits, ppm, S=S), a[S:S + Ms])
    # the realised missing share: within 5 binomial standard deviations of miss_ppm
    n, p = N * M, ppm * 1e-6
    miss = int((a == R).sum())
    print("missing %d of %d (expected %.1f, sd %.1f)" % (miss, n, n * p, np.sqrt(n * p * (1 - p))))
    assert abs(miss - n * p) <= 5 * np.sqrt(n * p * (1 - p))
    # no non-missing code equals the reserved one: miss_ppm = 0 has none at all, and differs from synth_dosage only where that
    # generator emits the reserved code (clamped one below)
    z, plain = synth.synth_dosage_na(N, M, 5, bits, 0), synth.synth_dosage(N, M, 5, bits)
    assert not np.any(z == R)
    diff = z != plain
    assert np.array_equal(diff, plain == R) and np.all(z[diff] == R - 1)
    big = synth.synth_dosage(4000, 300, 9, bits)
    if bits == 8:                                           # (the plain generator does emit 255: the clamp is not vacuous; 65535
        assert np.any(big == R)                             #  needs both 16-bit jitter fields at their top and is a rarity)
    zb = synth.synth_dosage_na(4000, 300, 9, bits, 0)
    assert np.array_equal(zb != big, big == R) and not np.any(zb == R)
    # the draw is independent of the code: the entries present at 30 000 ppm are the codes of miss_ppm = 0
    assert np.array_equal(a[a != R], z[a != R])
    assert np.all(synth.synth_dosage_na(50, 4, 1, bits, 1000000) == R)
    with pytest.raises(ValueError):
        synth.synth_dosage_na(4, 4, 1, bits, 1000001)
    with pytest.raises(ValueError):
        synth.synth_dosage_na(4, 4, 1, 12, 0)


def test_new_abi_names_are_declared_and_exported():
    with open(os.path.join(ROOT, "include", "gvamp.h")) as f:
        hdr = f.read()
    for name in NEW_NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in capi.EXPORTS
    assert re.search(r"#define\s+GV_ABI_VERSION\s+4\b", hdr)          # additions only
    assert "NO missing entries" not in hdr
    lib = os.path.join(ROOT, "gvamp_amd", "libgvamp.so")
    assert os.path.exists(lib), "libgvamp.so is built by build()"
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
    for name in NEW_NAMES:
        assert re.search(r"\bT %s$" % name, syms, re.M), name


def test_gvamp_main_real_checks_dosage_missing_before_device_work():
    exe = os.path.join(ROOT, "gvamp_amd", "gvamp_main_real")
    assert os.path.exists(exe), "gvamp_main_real is built by build() (gvamp_amd/csrc/host/Makefile)"
    for a in ("2", "-1", "yes"):
        r = subprocess.run([exe, "--dosage-missing", a], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "--dosage-missing" in r.stdout + r.stderr
