"""gv_screen_dev, capi.Shard.screen and gvamp_main_real --run-mode screen: the marginal association screen of
C = 5 phenotype columns on the two shapes of tests/bed_fixed_restatement.py -- three normal columns, one equal to a marker's
mean-imputed column plus 1e-3 noise (large |t|), one exactly collinear with a marker (the 1 - r^2 <= 0 rule).

Bars.  r and t: the restatement of tests/screen_restatement.py is evaluated in long double and in plain float64; the GPU (another
summation tree) is allowed 16 times the deviation of the float64 form, never less than 1e-12 (the rule of section 15, deviations taken
as it takes them: |dr| / (|r| + its sampling noise), |dt| / (|t| + 1)).  p: against the decimal reference of
tests/student_t_reference.py at the device's own t, |p / p_ref - 1| <= 2^-52 (1024 + 16 |ln p|), on at most 64 (marker, column)
entries picked by a fixed stride plus the smallest and the largest finite |t|.  The exactly collinear entry is decided by the last bit of
r on every side (t is +-inf or beyond 1e7, p is 0): it is held to that and left out of the deviations."""
import math
import os
import subprocess

import numpy as np
import pytest

import bed_fixed_restatement as bx
import screen_restatement as sr
import student_t_reference as st
from gvamp_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "gvamp_amd", "gvamp_main_real")
_CACHE = {}


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("GV_TUNE_CACHE", "0")
    for k in ("GV_ATXM_COLS", "GV_ATXM_KS", "GV_ATXM_KERNEL"):
        monkeypatch.delenv(k, raising=False)


def _case(name):
    """the case, its phenotypes and the two evaluations of the restatement: computed once, shared, never changed"""
    if name not in _CACHE:
        cs = bx.case(name)
        Y, near, coll = sr.phenotypes(cs)
        ref = sr.screen(cs["bed"], cs["N"], cs["M"], cs["present"], Y)
        r64 = sr.screen(cs["bed"], cs["N"], cs["M"], cs["present"], Y, dtype=np.float64)
        _CACHE[name] = (cs, Y, near, coll, ref, r64)
    return _CACHE[name]


def _shard(cs, kernel, m4=None, nonas=None):
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("GV_ATXM_KERNEL", kernel)
        sh = capi.Shard(cs["N"], cs["M"])
    sh.set_layout(False, 2)
    sh.upload_bed(cs["bed"])
    m4 = cs["m4"] if m4 is None else m4
    if m4 is not None:
        sh.set_mask(m4, cs["nonas"] if nonas is None else nonas)
    sh.compute_markers_statistics()
    return sh


def _envelope(p_ref):
    return 2.0 ** -52 * (1024.0 + 16.0 * abs(math.log(p_ref)))


@pytest.mark.parametrize("kernel", ["1", "0"], ids=["kernel", "fallback"])
@pytest.mark.parametrize("name", list(bx.SHAPES))
def test_r_t_p_against_the_restatement_and_the_decimal_tail(name, kernel):
    cs, Y, near, coll, ref, r64 = _case(name)
    n, M = cs["nonas"], cs["M"]
    with _shard(cs, kernel) as sh:
        r, t, p = sh.screen(Y)
        assert sh.atxm_info()["path"] == ("kernel" if kernel == "1" else "fallback") and sh.atxm_info()["columns"] == 5
    got = dict(r=r, t=t, p=p)
    # NaN rows are exactly MONO and ALLMISS, in all three outputs
    for k in ("r", "t", "p"):
        assert got[k].shape == (5, M)
        assert np.array_equal(np.nonzero(np.isnan(got[k]).any(axis=0))[0], [bx.MONO, bx.ALLMISS]), k
        assert np.all(np.isnan(got[k][:, [bx.MONO, bx.ALLMISS]])), k
    # the exactly collinear entry: the rule, or the last bit of r short of it
    assert r[4, coll] < -1 + 1e-12 and (t[4, coll] == -np.inf or t[4, coll] < -1e7) and p[4, coll] == 0.0
    assert r[3, near] > 0.99999 and t[3, near] > 1e3
    skip = [(4, coll)]
    dev64, devg = sr.deviation(r64, ref, n, skip), sr.deviation(got, ref, n, skip)
    for k in ("r", "t"):
        bound = max(16.0 * dev64[k], 1e-12)
        print("%s %s %s: float64 dev %.3e  GPU dev %.3e  bound %.3e" % (name, kernel, k, dev64[k], devg[k], bound))
        assert devg[k] <= bound, (k, devg[k], bound)
    keep = np.isfinite(t)
    assert np.all(np.sign(t[keep]) == np.sign(r[keep]))
    # p at the device's own t against the decimal reference
    flat = [(c, m) for c in range(5) for m in range(M) if np.isfinite(t[c, m]) and t[c, m] != 0.0]
    fin = sorted(flat, key=lambda cm: abs(t[cm]))
    rows = flat[::max(1, len(flat) // 60)][:62] + [fin[0], fin[-1]]
    assert len(rows) <= 64
    worst = 0.0
    for c, m in rows:
        pr = st.tail(float(t[c, m]), n - 2)
        if pr is None or float(pr) < 1e-290:
            assert 0.0 <= p[c, m] <= 1e-289, (c, m, t[c, m], p[c, m])
            continue
        pr = float(pr)
        share = abs(p[c, m] / pr - 1.0) / _envelope(pr)
        worst = max(worst, share)
        assert share <= 1.0, (c, m, t[c, m], p[c, m], pr)
    print("%s %s p: worst share of the envelope %.3f over %d entries" % (name, kernel, worst, len(rows)))


def test_screen_dev_without_t_and_p_and_its_refusals():
    cs, Y, near, coll, ref, r64 = _case("ragged")
    with _shard(cs, "1") as sh:
        r, t, p = sh.screen(Y)
        U = sh.screen_prepare(Y)
        us, rs = [sh.vecN(u) for u in U], [sh.vecM() for _ in U]
        sh.screen_dev(us, rs)                                        # t and p may be NULL arrays
        assert all(np.array_equal(v.download().view(np.uint64), r[j].view(np.uint64)) for j, v in enumerate(rs))
        sh.screen_dev([], [])
        with pytest.raises(capi.GvError, match="two outputs are the same vector"):
            sh.screen_dev(us[:2], rs[:2], [rs[0], rs[3]], None)
        with pytest.raises(capi.GvError, match="u must be N-space, out M-space"):
            sh.screen_dev([rs[0]], [rs[1]])
        with pytest.raises(capi.GvError, match="arrays of column handles are NULL"):
            sh.screen_dev(None, rs)
        sh.screen_dev(us, rs)
        assert np.array_equal(rs[1].download().view(np.uint64), r[1].view(np.uint64))
    # methylation and dosage data: refused by message; fewer than 3 phenotyped individuals: refused
    for what in ("meth", "dosage8"):
        with capi.Shard(64, 32) as sh:
            if what == "meth":
                sh.synth_meth(3)
            else:
                sh.synth_dosage(3, 8)
            with pytest.raises(capi.GvError, match="methylation or dosage"):
                sh.screen_dev([sh.vecN().fill(0.0)], [sh.vecM()])
    with capi.Shard(8, 64) as sh:
        sh.set_layout(False, 2)
        sh.synth_bed(3)
        sh.set_mask(np.array([0x03, 0x00], dtype=np.uint8), 2)
        sh.compute_markers_statistics()
        with pytest.raises(capi.GvError, match="fewer than 3"):
            sh.screen_dev([sh.vecN().fill(0.0)], [sh.vecM()])


def test_a_widened_na_pattern_equals_a_fresh_context_on_the_merged_mask():
    cs, Y, near, coll, ref, r64 = _case("ragged")
    N = cs["N"]
    pres = cs["present"].copy()
    pres[np.nonzero(pres)[0][3::17]] = False                        # the merged mask leaves out more individuals
    m4 = np.zeros((N + 3) // 4, dtype=np.uint8)
    idx = np.nonzero(pres)[0]
    np.bitwise_or.at(m4, idx >> 2, (1 << (idx & 3)).astype(np.uint8))
    Ym = Y.copy()
    Ym[:, ~pres] = np.nan
    with _shard(cs, "1") as sh:
        with pytest.raises(capi.GvError, match="is NA at an individual"):
            sh.screen(Ym)                                            # an NA inside the context's mask is refused
        sh.set_mask(m4, int(pres.sum()))
        sh.compute_markers_statistics()
        got = sh.screen(Y)                                           # the columns know fewer NAs than the mask: the mask decides
    with _shard(cs, "1", m4=m4, nonas=int(pres.sum())) as sh:
        fresh = sh.screen(Ym)
    for a, b in zip(got, fresh):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert not np.array_equal(got[0], _screen_cached("ragged")[0], equal_nan=True)


def _screen_cached(name):
    key = ("gpu", name)
    if key not in _CACHE:
        cs, Y = _case(name)[:2]
        with _shard(cs, "1") as sh:
            _CACHE[key] = sh.screen(Y)
    return _CACHE[key]


def test_driver_equals_the_python_result(tmp_path):
    cs, Y, near, coll, ref, r64 = _case("ragged")
    N, M = cs["N"], cs["M"]
    mb = (N + 3) // 4
    bed = str(tmp_path / "toy.bed")
    with open(bed, "wb") as f:
        f.write(bytes([0x6C, 0x1B, 0x01]))
        f.write(np.asarray(cs["bed"], dtype=np.uint8).reshape(M, mb).tobytes())
    # three phen files (the three normal columns) with different NA patterns: the complete cases are their intersection
    rng = np.random.default_rng(3)
    cols = [0, 1, 2]
    Yf = Y[cols].copy()
    Yf[:, ~cs["present"]] = rng.standard_normal((3, int((~cs["present"]).sum())))      # the files decide who is NA
    nas = [rng.choice(N, 9, replace=False) for _ in cols]
    files = []
    for k, na in enumerate(nas):
        Yf[k, na] = np.nan
        path = str(tmp_path / ("p%d.phen" % k))
        with open(path, "w") as f:
            for n in range(N):
                f.write("f%d i%d %s\n" % (n, n, "NA" if np.isnan(Yf[k, n]) else repr(float(Yf[k, n]))))
        files.append(path)
    out = str(tmp_path / "out") + "/"
    os.makedirs(out, exist_ok=True)
    cmd = [EXE, "--run-mode", "screen", "--bed-file", bed, "--N", str(N), "--Mt", str(M), "--phen-files", ",".join(files), "--out-dir", out,
           "--out-name", "t", "--screen-cols", "2"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "screen: 3 phenotypes" in res.stdout
    merged = ~np.isnan(Yf).any(axis=0)
    m4 = np.zeros(mb, dtype=np.uint8)
    idx = np.nonzero(merged)[0]
    np.bitwise_or.at(m4, idx >> 2, (1 << (idx & 3)).astype(np.uint8))
    with _shard(cs, "0", m4=m4, nonas=int(merged.sum())) as sh:
        want = sh.screen(Yf)
    for k, tag in enumerate("rtp"):
        got = np.fromfile(out + "t_screen_%s.bin" % tag).reshape(3, M)
        assert np.array_equal(np.isnan(got), np.isnan(want[k])), tag
        assert np.array_equal(np.nonzero(np.isnan(got).any(axis=0))[0], [bx.MONO, bx.ALLMISS]), tag
        ok = ~np.isnan(want[k])
        assert np.all(np.isfinite(want[k][ok]))
        # to 1e-12: relative for p, against |value| + 1 for r and t
        scale = np.abs(want[k][ok]) + (0.0 if tag == "p" else 1.0)
        assert np.all(np.abs(got[ok] - want[k][ok]) <= 1e-12 * scale), (tag, float(np.max(np.abs(got[ok] - want[k][ok]) / scale)))
