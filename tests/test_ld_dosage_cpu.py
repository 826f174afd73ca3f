"""The LD of 8-bit dosage codes (gv_set_ld_dosage), the parts that need no GPU: the integer restatement of
tests/ld_dosage_restatement.py held to np.corrcoef, to the bed restatement, and to a long-double evaluation that centres first; the
float64 four-term form of section 16 shown to lose what the integer form keeps (the reason for the integer form); the inputs of the
int32-bound test; and the new C-ABI names."""
import os
import re

import numpy as np

import ld_dosage_restatement as ldd
import ld_restatement as ldr
import precond_restatement as pr
from gvamp_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
NEW_NAMES = ("gv_set_ld_dosage", "gv_get_ld_dosage")


def test_complete_data_equal_corrcoef():
    N, M = 403, 300
    codes = synth.synth_dosage(N, M, 3, 8)
    r = ldd.ld(codes)["r"]
    want = np.corrcoef(codes.astype(np.float64))
    print("max |r - corrcoef| = %.3e" % np.max(np.abs(r - want)))
    assert np.max(np.abs(r - want)) <= 1e-14


def test_a_bed_written_as_codes_equals_the_bed_restatement():
    N, M = 403, 300
    bed = synth.synth_bed(N, M, seed=3, miss_ppm=20000, ld_block=48, ld_ppm=900000)
    a, b = pr.decode(bed, N, M)
    codes = np.where(np.asarray(b).T != 0, np.asarray(a).T, 255).astype(np.uint8)        # 0 / 1 / 2, 255 at a missing genotype
    na = np.ones(N)
    na[::7] = 0.0
    ref = ldr.ld(bed, N, M, 40, na=na)
    got = ldd.ld(codes, na, missing=True)
    print("max |r - bed restatement| = %.3e" % np.max(np.abs(got["r"] - ref["r"])))
    assert np.array_equal(got["poly"], ref["poly"])
    assert np.max(np.abs(got["r"] - ref["r"])) <= 1e-14


def _centre_first(codes):
    """r in long double, centring before multiplying"""
    d = codes.astype(LD)
    d = d - d.mean(1, keepdims=True)
    C = d @ d.T
    v = np.diag(C)
    return C / np.sqrt(v[:, None] * v[None, :])


def _four_term_f64(codes):
    """section 16's form on the biased codes in float64: VV - m_k VP_jk - m_j VP_kj + m_j m_k PP with m = T / c"""
    s = ldd.sums(codes)
    VV, VP, PP = (s[k].astype(np.float64) for k in ("VV", "VP", "PP"))
    m = s["T"].astype(np.float64) / s["c"].astype(np.float64)
    C = VV - m[None, :] * VP - m[:, None] * VP.T + np.outer(m, m) * PP
    v = np.diag(C)
    return C / np.sqrt(v[:, None] * v[None, :])


def test_rare_variant_rows_integer_form_against_long_double_and_the_four_term_form():
    codes = ldd.rare_rows()
    ref = _centre_first(codes)
    off = ~np.eye(codes.shape[0], dtype=bool)
    r = ldd.ld(codes)["r"]
    e_int = float(np.max(np.abs(r.astype(LD) - ref)[off]))
    e_f64 = float(np.max(np.abs(_four_term_f64(codes).astype(LD) - ref)[off]))
    print("rare-variant rows: integer form %.3e, float64 four-term form %.3e from long double" % (e_int, e_f64))
    assert e_int <= 1e-15
    assert e_f64 > 1e-11            # what the integer form is for


def test_the_bound_inputs_wrap_an_unsegmented_int32_sum():
    codes = ldd.bound_case()
    assert codes.shape == (70, 140000)
    s = ldd.sums(codes[:2])
    assert int(s["VV"][0, 0]) == 2275910000 and int(s["VV"][0, 1]) == -2275840000
    assert s["VV"][0, 0] > 2 ** 31 - 1 and s["VV"][0, 1] < -2 ** 31
    assert 131071 * 16384 <= 2 ** 31 - 1 < 131072 * 16384          # one segment of the kernel cannot wrap, one entry more could
    r = ldd.ld(codes[:2])["r"]
    assert r[0, 1] == -1.0


def test_constant_and_all_missing_rows_cancel_exactly():
    N = 77
    codes = np.random.default_rng(1).integers(0, 255, size=(4, N), dtype=np.uint8)
    codes[1] = 253
    codes[2] = 255
    na = np.ones(N)
    na[::5] = 0.0
    got = ldd.ld(codes, na, missing=True)
    assert list(got["poly"]) == [True, False, False, True]
    assert got["X"][1, 1] == 0 and got["X"][2, 2] == 0 and np.all(got["r"][1] == 0) and np.all(got["r"][2] == 0)


def test_new_names_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "gvamp.h")).read()
    for n in NEW_NAMES:
        assert re.search(r"\bint %s\(" % n, hdr), n
        assert n in capi.EXPORTS, n
    assert re.search(r"#define GV_ABI_VERSION 4\b", hdr)
    assert hasattr(capi.Shard, "set_ld_dosage") and hasattr(capi.Shard, "get_ld_dosage")
