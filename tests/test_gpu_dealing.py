"""Work items of the streaming kernels dealt by ticket (gv_mfma.h: item_cells, Deal) against the block-index mapping of the same binary
(GV_DEAL=0, read by gv_create): two contexts in one process, the same data, every result compared with array_equal.  The partial sums
are exact integers and every item writes the slots it always wrote, so not one bit may differ -- and the ticket counter is never reset,
so a launch whose base is off by one hands out the wrong items to every launch after it: each case ends with further products."""
import contextlib
import os

import numpy as np
import pytest

from gvamp_amd import capi, synth

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    for k, v in kw.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _shard(deal, N, M, layout, seed=7, miss_ppm=10000, fna=0.02, mode=1):
    with _env(GV_DEAL=None if deal else 0, GV_TUNE_CACHE=0):
        sh = capi.Shard(N, M)                       # (GV_DEAL is read here, per context)
    sh.set_layout(False, layout)                    # 1: two stripe sets, 2: one tile layout
    sh.set_kernel_mode(mode)
    sh.upload_bed(synth.synth_bed(N, M, seed=seed, miss_ppm=miss_ppm))
    if fna > 0:
        present = np.random.default_rng(N).random(N) >= fna
        m4 = np.zeros((N + 3) // 4, dtype=np.uint8)
        for n in np.nonzero(present)[0]:
            m4[n >> 2] |= 1 << (n & 3)
        sh.set_mask(m4, int(present.sum()))
    sh.compute_markers_statistics()
    return sh


def _products(sh, M, seed=1):
    """Ax, ATx, the two-vector forms and lmmse_mult, device-vector and host-pointer forms"""
    rng = np.random.default_rng(seed)
    xa, xb = rng.standard_normal(M), rng.standard_normal(M) * 1e-3
    x, x2 = sh.vecM(xa), sh.vecM(xb)
    z, z2, w, w2 = sh.vecN(), sh.vecN(), sh.vecM(), sh.vecM()
    out = []
    sh.ax_dev(x, z)
    sh.atx_dev(z, w)
    out += [z.download(), w.download()]
    sh.ax2_dev(x, x2, z, z2)
    sh.atx2_dev(z, z2, w, w2)
    out += [z.download(), z2.download(), w.download(), w2.download()]
    sh.lmmse_mult(x, 1.7, 0.3, w)
    out.append(w.download())
    zh = sh.Ax(xa)
    out += [zh, sh.ATx(zh)]
    return out


def _same(a, b, what):
    assert len(a) == len(b)
    for k, (p, q) in enumerate(zip(a, b)):
        assert np.array_equal(p, q, equal_nan=True), "%s: result %d differs" % (what, k)
        assert np.any(p != 0), (what, k)            # (a comparison of two all-zero outputs would prove nothing)


# pinned decompositions: (label, keyword arguments of set_decomp); admissible on both sides of both layouts at N = 4101 x M = 6007
DECOMPS = [
    ("library pick", None),
    ("uniform ks 3, skewed under the block-index mapping", dict(ks=3, xcd_skew=0.02)),
    ("tapered ks 4", dict(ks=4, taper=0.9, prio=1)),
    ("geometric ks 3", dict(ks=3, geo=0.5, prio=1)),
    ("balanced", dict(balanced_cells=9, prio=1)),
    ("hybrid", dict(balanced_cells=9, whole_quads=3, prio=1)),
    ("hybrid, two workgroups per CU", dict(balanced_cells=8, whole_quads=2, prio=1, wgs_per_cu=2)),
]


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("layout", [1, 2])
def test_dealt_items_give_the_same_bits(layout, mode):
    N, M = 4101, 6007                               # ragged in both directions; missing genotypes and masked individuals
    with _shard(True, N, M, layout, mode=mode) as a, _shard(False, N, M, layout, mode=mode) as b:
        ref = None
        for label, kw in DECOMPS:
            if kw is not None:
                for sh in (a, b):
                    for cls in range(4):
                        sh.set_decomp(cls, **kw)
                assert a.decomp() == b.decomp()     # gv_get_decomp echoes what was set, xcd_skew included
            ra, rb = _products(a, M), _products(b, M)
            _same(ra, rb, "layout %d mode %d %s" % (layout, mode, label))
            if ref is None:
                ref = ra
            _same(ra, ref, "layout %d mode %d %s against the library pick" % (layout, mode, label))


@pytest.mark.parametrize("layout", [1, 2])
def test_fewer_than_eight_items_and_an_empty_shard(layout):
    N, M = 300, 200                                 # ATx: one quad; Ax: one or two -- every launch is mostly spare workgroups
    with _shard(True, N, M, layout) as a, _shard(False, N, M, layout) as b:
        for _ in range(3):
            _same(_products(a, M), _products(b, M), "layout %d, small" % layout)
    for deal in (True, False):
        with _env(GV_DEAL=None if deal else 0):
            sh = capi.Shard(100, 0, Mt=10, S=10)
        with sh:
            sh.set_layout(False, layout)
            sh.upload_bed(np.zeros(0, dtype=np.uint8))
            sh.compute_markers_statistics()
            z = sh.Ax(np.zeros(0))
            assert z.shape == (100,) and np.all(z == 0)
            assert sh.ATx(np.zeros(100)).shape == (0,)


@pytest.mark.parametrize("layout", [1, 2])
def test_people_statistics_pvalues_and_chunked_ax(layout):
    N, M = 4101, 6007
    rng = np.random.default_rng(3)
    x1 = rng.standard_normal(M) * (rng.random(M) < 0.05) * 3.0
    noise = rng.standard_normal(N)
    chrom = np.sort(rng.integers(1, 24, M)).astype(np.int32)
    with _shard(True, N, M, layout) as a, _shard(False, N, M, layout) as b:
        def run(sh):
            out = list(sh.compute_people_statistics())
            dx, dz = sh.vecM(x1), sh.vecN()
            sh.ax_dev(dx, dz)
            z1 = dz.download()
            dy = sh.vecN(z1 + np.concatenate([noise, np.zeros(z1.size - N)]) * (z1 != 0))
            out += [z1, sh.pvals_calc(dz, dy, dx), sh.pvals_calc(dz, dy, dx, chrom=chrom)]
            return out + _products(sh, M, seed=5)
        _same(run(a), run(b), "layout %d statistics and p-values" % layout)
        plain = _products(a, M, seed=9)
        for sh in (a, b):                           # gv_set_overlap on the forced-multi hook: Ax in four ax_rows chunks
            sh.force_multi(1, 0)
            sh.set_overlap(4)
        try:
            ca, cb = _products(a, M, seed=9), _products(b, M, seed=9)
        finally:
            for sh in (a, b):
                sh.force_multi(0)
                sh.set_overlap(0)
        _same(ca, cb, "layout %d chunked Ax" % layout)
        _same(ca, plain, "layout %d chunked Ax against the undivided pass" % layout)
        _same(_products(a, M, seed=9), plain, "layout %d after the chunked passes" % layout)


@pytest.mark.parametrize("layout", [1, 2])
def test_counter_survives_the_skipped_passes_of_a_device_resident_cg(layout):
    """A well-conditioned system converges in a few steps while the host has already enqueued more: the streaming launches of the
    steps past convergence return at their `go` test -- after drawing their tickets, or the products that follow would run the
    wrong items."""
    N, M = 4101, 6007
    rng = np.random.default_rng(11)
    v, vb = rng.standard_normal(M), rng.standard_normal(M)
    with _shard(True, N, M, layout) as a, _shard(False, N, M, layout) as b:
        def run(sh):
            dv, dvb, mu, mub = sh.vecM(v), sh.vecM(vb), sh.vecM(), sh.vecM()
            out = []
            for tau, gam2, it in ((0.05, 4.0, 60), (2.0, 1.35, 60)):
                st, rr = sh.cg_solve(dv, None, tau, gam2, 1, it, mu)
                assert 0 < st.iters < it            # it converged: steps enqueued beyond it were dropped on the device
                out += [mu.download(), rr, np.array([st.iters], dtype=np.float64)]
                out += _products(sh, M, seed=13)
                (sa, ra), (sb, rb) = sh.cg_solve2(dv, None, dvb, tau, gam2, it, mu, mub)
                assert 0 < sa.iters < it and 0 < sb.iters < it
                out += [mu.download(), mub.download(), ra, rb]
                out += _products(sh, M, seed=17)
            return out
        _same(run(a), run(b), "layout %d CG and the products behind it" % layout)
        _same(run(a), run(b), "layout %d CG, again on the same contexts" % layout)
