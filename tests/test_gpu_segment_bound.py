"""The int32 bound of the Ax side at the smallest shape that can break it: N = 8 individuals x M = 6 400 000 markers (12.8 MB of .bed
rows).  A work item of the streaming kernels adds up to 512 per marker into an int32 digit sum (gv_mfma.h, ax_bound_ok), so a K-segment
of more than 4 194 303 markers can wrap -- and two segments are enough by count at this M while the first segment of `ks 2 geo 0.5`,
`ks 2 geo 0.35`, `ks 2 taper 0.5` and `ks 2 taper 0.9` is longer than that.

The adversarial input makes every marker of a segment pull the same way: marker 0 is monomorphic a = 2 and carries x = 2^53, which
pins the quantisation multiplier to 1; every other marker is all-missing and carries x = -0x808080808080, whose balanced base-256
digits are -128 in columns 0..5, as is digit 0 of e = -3 c.  Each missing entry adds 3 * (-128) + (-128) = -512 to the column-0 sum;
the exact product is 0 for every individual (3 c + e = 0 term by term in integers, and (2 - mave) = 0 on marker 0), so the kernels'
answer is exactly 0.0 unless a sum wraps."""
import contextlib

import numpy as np
import pytest

from gvamp_amd import capi

pytestmark = pytest.mark.gpu
TOL = 1e-12
N, M = 8, 6400000
I32_MAX = 2 ** 31 - 1
LIMIT = I32_MAX // 512           # 4 194 303 markers
MIN_KS = 2                       # ceil(M * 512 / (2^31 - 1)), and two halves of 3 200 000 markers keep the bound on both layouts
X_ADV = -141289400074368.0       # -0x808080808080
LAYOUTS = [pytest.param(1, id="two-stripe-sets"), pytest.param(2, id="tile")]       # gv_set_layout(raw, stripes)
KB_MARKERS = {1: 256, 2: 64}     # markers per K-block of the Ax side
PINS = (dict(ks=2, taper=0.9), dict(ks=2, taper=0.5), dict(ks=2, geo=0.35), dict(ks=2, geo=0.5))
ENV = ("GV_AUTOTUNE", "GV_KS_M", "GV_KS_N", "GV_SK_M", "GV_SK_N", "GV_HY_M", "GV_HY_N", "GV_PRIO", "GV_TAPER", "GV_GEO", "GV_DEAL",
       "GV_TUNE_GEO", "GV_TUNE_BUILTIN")


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("GV_TUNE_CACHE", "0")         # picks are neither read from nor left in the user's cache file


def f32(v):
    return float(np.float32(v))


def segments(ks, taper, geo, xskew, nkb, deal, parity):
    """K-block boundaries of a uniform split: gvm::make_bounds restated (gv_mfma.h; Decomp's fields are floats)"""
    taper, geo, xskew = f32(taper), f32(geo), (0.0 if deal else f32(xskew))
    w = []
    for j in range(ks):
        if geo > 0 and ks > 1:
            w.append(w[-1] * geo if j else 1.0)
        else:
            w.append(1.0 + taper * (ks - 1 - 2 * j) / (ks - 1) if ks > 1 else 1.0)
    v = [w[j] * (1.0 + xskew if (parity + j) & 1 else 1.0 - xskew) for j in range(ks)]
    tot = 0.0
    for t in v:
        tot += t
    b, acc = [0], 0.0
    for j in range(ks):
        acc += v[j]
        e = int(nkb * acc / tot + 0.5)
        b.append(min(max(e, b[j] + 1), nkb - (ks - 1 - j)))
    b[ks] = nkb
    if deal:
        ln = sorted((y - x for x, y in zip(b, b[1:])), reverse=True)
        b = [0]
        for t in ln:
            b.append(b[-1] + t)
    return b


def longest_segment(spec, stripes):
    """markers of the longest segment of a uniform split, over both mappings and both quad parities"""
    kbm = KB_MARKERS[stripes]
    nkb = -(-M // kbm)
    longest = 0
    for deal in (False, True):
        for parity in (0, 1):
            b = segments(spec["ks"], spec.get("taper", 0.0), spec.get("geo", 0.0), spec.get("xcd_skew", 0.0), nkb, deal, parity)
            longest = max([longest] + [min(hi * kbm, M) - lo * kbm for lo, hi in zip(b, b[1:])])
    return longest


def keeps_bound(spec, stripes):
    return "balanced_cells" not in spec and 1 <= spec["ks"] <= 64 and longest_segment(spec, stripes) * 512 <= I32_MAX


def adversarial(madv):
    """.bed rows and vector: marker 0 monomorphic a = 2 with x = 2^53, markers 1 .. madv - 1 all-missing with x = -0x808080808080"""
    bed = np.full((madv, 2), 0x55, dtype=np.uint8)
    bed[0, :] = 0x00
    x = np.full(madv, X_ADV)
    x[0] = 2.0 ** 53
    return bed, x


@pytest.fixture(scope="module")
def adv():
    bed, x = adversarial(M)
    bed.setflags(write=False)
    x.setflags(write=False)
    return bed, x


def digit0(v, mult):
    """balanced base-256 digit 0 of q = rint(v * mult), by the definition at the head of gv_mfma.hip"""
    q = np.rint(v * mult).astype(np.int64)
    return ((q + 128) & 0xFF) - 128


def column0_prefix_sums(bed, x, mave, msig):
    """int64 prefix sums over the markers of what ONE row (individual 0) adds to the int32 sum of digit column 0 in an Ax pass of kernel
    mode 1: r' * digit0(c) + miss * digit0(e), with c = msig x, e = (mave - 3) c and one exponent for both (k_prep_ax, k_quant)"""
    c = msig * x
    e = (mave - 3.0) * c
    amax = max(np.abs(c).max(), np.abs(e).max())
    ex = int(np.frexp(amax)[1])                      # 2^(ex-1) <= amax < 2^ex
    mult = 2.0 ** (54 - ex)
    code = bed[:, 0] & 3                             # PLINK: 00 a = 2, 10 a = 1, 11 a = 0, 01 missing
    rprime = np.array([2, 3, 1, 0], dtype=np.int64)[code]
    miss = (code == 1).astype(np.int64)
    return mult, np.cumsum(rprime * digit0(c, mult) + miss * digit0(e, mult))


@contextlib.contextmanager
def shard(bed, stripes, mode=1):
    with capi.Shard(N, M) as sh:
        sh.set_layout(False, stripes)
        sh.set_kernel_mode(mode)
        sh.upload_bed(bed.reshape(-1))
        sh.compute_markers_statistics()
        yield sh


def check_adversarial(sh, bed, x, stripes):
    """the input is what the module's docstring says it is, on THIS shard's statistics: the test is vacuous otherwise"""
    mave, msig = sh.marker_stats()
    assert mave[0] == 2.0 and msig[0] == 1.0 and np.all(mave[1:] == 0.0) and np.all(msig[1:] == 1.0)
    mult, cum = column0_prefix_sums(bed, x, mave, msig)
    assert mult == 1.0
    kbm, nkb = KB_MARKERS[stripes], -(-M // KB_MARKERS[stripes])
    for spec in PINS:
        for deal in (False, True):
            first = segments(spec["ks"], spec.get("taper", 0.0), spec.get("geo", 0.0), 0.0, nkb, deal, 0)[1] * kbm
            assert first >= 4194305 and cum[first - 1] < -2 ** 31, (spec, first, int(cum[first - 1]))
    for lo, hi in ((0, M // 2), (M // 2, M)):         # ... and the two equal halves stay inside int32
        assert -2 ** 31 <= cum[hi - 1] - (cum[lo - 1] if lo else 0) <= I32_MAX


def ax_products(sh, vx, vr):
    """one-vector Ax of the adversarial vector, two-vector Ax with it in both slots and in either slot beside a random vector"""
    o = [sh.vecN() for _ in range(7)]
    sh.ax_dev(vx, o[0])
    sh.ax2_dev(vx, vx, o[1], o[2])
    sh.ax2_dev(vx, vr, o[3], o[4])
    sh.ax2_dev(vr, vx, o[5], o[6])
    out = [v.download() for v in o]
    for v in o:
        v.free()
    return out


ADV_SLOTS = (0, 1, 2, 3, 6)      # outputs of ax_products that belong to the adversarial vector


@pytest.mark.parametrize("deal", ["1", "0"])
@pytest.mark.parametrize("stripes", LAYOUTS)
def test_inadmissible_pins_are_refused_and_the_product_stays_exact(monkeypatch, adv, stripes, deal):
    bed, x = adv
    monkeypatch.setenv("GV_DEAL", deal)
    with shard(bed, stripes) as sh:
        check_adversarial(sh, bed, x, stripes)
        assert np.all(sh.Ax(x) == 0.0)
        keep = sh.decomp()
        for cls in ("ax", "ax2"):
            assert keeps_bound(keep[cls], stripes), keep
            for spec in PINS:
                assert not keeps_bound(spec, stripes)
                with pytest.raises(capi.GvError, match="not admissible"):
                    sh.set_decomp(cls, **spec)
        assert sh.decomp() == keep
        vx, vr = sh.vecM(x), sh.vecM(np.random.default_rng(1).standard_normal(M))
        z = sh.Ax(x)
        assert z.shape == (N,) and np.all(z == 0.0), z
        out = ax_products(sh, vx, vr)
        for k in ADV_SLOTS:
            assert np.all(out[k] == 0.0), (k, out[k][:N])
        assert np.array_equal(out[4], out[5])        # the random vector's product does not depend on its slot


@pytest.mark.parametrize("stripes", LAYOUTS)
def test_whatever_is_admitted_is_exact(adv, stripes):
    bed, x = adv
    specs = [dict(ks=ks, geo=geo, taper=taper) for ks in (2, 3, 4, 6, 8, 12, 24, 64) for geo in (0.0, 0.35, 0.5, 0.6, 0.65, 0.7, 0.8)
             for taper in (0.0, 0.5) if not (geo and taper)]
    assert len(specs) == 64
    with shard(bed, stripes) as sh:
        vx, vr = sh.vecM(x), sh.vecM(np.random.default_rng(2).standard_normal(M))

        def run():
            return ax_products(sh, vx, vr) + list(sh.compute_people_statistics())

        run()                                        # (the automatic pick is made before anything is pinned)
        for cls in ("ax", "ax2"):
            sh.set_decomp(cls, ks=MIN_KS)
            assert sh.decomp()[cls]["ks"] == MIN_KS and sh.decomp()[cls]["taper"] == 0.0
        ref = run()
        for k in ADV_SLOTS:
            assert np.all(ref[k] == 0.0), k
        admitted = refused = 0
        for spec in specs:
            ok = keeps_bound(spec, stripes)
            try:
                for cls in ("ax", "ax2"):
                    sh.set_decomp(cls, **spec)
            except capi.GvError as e:
                # refused: for the int32 bound where the restated boundaries break it, for another reason (say so) where they do not
                assert "not admissible" in str(e) and ("int32" in str(e)) == (not ok), (spec, str(e))
                refused += 1
                continue
            assert ok, spec
            admitted += 1
            got = run()
            for k in ADV_SLOTS:
                assert np.all(got[k] == 0.0), (spec, k, got[k][:N])
            for a, b in zip(ref, got):
                assert np.array_equal(a, b, equal_nan=True), spec
        assert admitted >= 10 and refused >= 4, (admitted, refused)


@pytest.mark.parametrize("env", [{}, {"GV_AUTOTUNE": "0"}, {"GV_KS_N": "2", "GV_TAPER": "0.9"}], ids=["autotune", "model", "override"])
@pytest.mark.parametrize("stripes", LAYOUTS)
def test_the_automatic_path_keeps_the_bound(monkeypatch, adv, stripes, env):
    bed, x = adv
    monkeypatch.setenv("GV_TUNE_BUILTIN", "0")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with shard(bed, stripes) as sh:
        z = sh.Ax(x)
        vx, vr = sh.vecM(x), sh.vecM(np.random.default_rng(3).standard_normal(M))
        out = ax_products(sh, vx, vr)
        d = sh.decomp()
        assert sh.tune_info()[1] == ("fixed" if "GV_AUTOTUNE" in env else "measured"), sh.tune_info()
        for cls in ("ax", "ax2"):
            assert d[cls]["tuned"] and keeps_bound(d[cls], stripes), d
            if "GV_KS_N" in env:                     # the override asks for a first segment of 95 % of the markers: it must not take
                assert not (d[cls]["ks"] == 2 and d[cls]["taper"] == 0.9), d
        assert np.all(z == 0.0), z
        for k in ADV_SLOTS:
            assert np.all(out[k] == 0.0), (k, d, out[k][:N])


@pytest.fixture(scope="module")
def mixed(oracle):
    """the first 4 800 000 markers adversarial, the rest random genotypes with 2 % missing and x ~ N(0, 1) * 2^40; oracle products"""
    madv = 4800000
    rng = np.random.default_rng(11)
    bed_a, x_a = adversarial(madv)
    code = rng.choice(np.array([0, 2, 3, 1], dtype=np.uint8), size=(M - madv, N), p=[0.245, 0.49, 0.245, 0.02])
    bed_r = (code.reshape(-1, 2, 4) << (2 * np.arange(4, dtype=np.uint8))).sum(axis=2).astype(np.uint8)
    bed = np.concatenate([bed_a, bed_r])
    x = np.concatenate([x_a, rng.standard_normal(M - madv) * 2.0 ** 40])
    p = rng.standard_normal(N)
    mave, msig = oracle.marker_stats(bed.reshape(-1), N, M)
    oz = oracle.ax(bed.reshape(-1), N, M, mave, msig, x)
    ow = oracle.atx(bed.reshape(-1), N, M, mave, msig, p)
    for a in (bed, x, p, mave, msig, oz, ow):
        a.setflags(write=False)
    return bed, x, p, mave, msig, oz, ow


@pytest.mark.parametrize("stripes", LAYOUTS)
def test_a_non_degenerate_product_at_this_shape(mixed, stripes):
    bed, x, p, o_mave, o_msig, oz, ow = mixed
    with shard(bed, stripes) as sh:
        mave, msig = sh.marker_stats()
        assert np.allclose(mave, o_mave, rtol=1e-13, atol=1e-15) and np.allclose(msig, o_msig, rtol=1e-12, atol=0)
        z = sh.Ax(x)
        # the accuracy contract of kernel mode 1 (include/gvamp.h; test_fixed_point_per_entry_bound_on_adversarial_dynamic_range)
        bound = M * 2.0 ** -50 * np.max(np.abs(msig * x)) / np.sqrt(N)
        err = np.abs(z - oz)
        print("Ax: max |err| %.3e, bound %.3e, max |Ax| %.3e" % (err.max(), bound, np.abs(oz).max()))
        assert bound < 2.0 ** 32 / np.sqrt(N) / 8      # (a wrapped column-0 sum is 2^32 / sqrt(N) off: the bound would see it)
        assert np.all(err <= bound), (err.max(), bound)
        assert np.abs(oz).max() > 1e3 * bound
        w = sh.ATx(p)
        rel = np.linalg.norm(w - ow) / np.linalg.norm(ow)
        print("ATx: rel l2 err %.3e" % rel)
        assert rel < TOL
        v = sh.vecM(x)                               # 51 MB: six trips through the 8 MiB staging buffer, each way
        assert np.array_equal(v.download(), x)
        for cls in ("ax", "ax2"):
            assert keeps_bound(sh.decomp()[cls], stripes), sh.decomp()


@pytest.mark.parametrize("stripes", LAYOUTS)
def test_kernel_mode_2_is_exact_on_the_adversarial_vector(adv, stripes):
    """two-level fixed point: a missing genotype is 0 in both planes (a' and present), so no entry adds more than 384 and these
    markers add nothing at all; the automatic decomposition is the Ax side's all the same"""
    bed, x = adv
    with shard(bed, stripes, mode=2) as sh:
        z = sh.Ax(x)
        assert z.shape == (N,) and np.all(z == 0.0), z
        for cls in ("ax", "ax2"):
            assert keeps_bound(sh.decomp()[cls], stripes), sh.decomp()
