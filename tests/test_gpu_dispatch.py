"""Characterisation of the product dispatch (gv_matvec.hip: ax_pass / atx_pass / exchange_n): what every data::Ax / data::ATx
entry point adds to the counters, and that a two-vector pass, a forced multi-rank pass, an overlapped pass and the pass of an
empty shard give the same bits as the plain one-vector passes.

The counter tables below are LITERALS: they were recorded from the commit before the four dispatchers were merged into two
(fe3f1b6) and are never computed from the library under test.  Columns: n_ax, n_ax_pass, n_atx, n_atx_pass, n_allreduce,
n_ax_kernel, n_atx_kernel, cumulative after each call of SEQUENCE.  What they pin down:
  * n_ax / n_atx advance by the number of vectors;
  * a two-vector product is ONE pass in kernel mode 1 and on methylation data, two complete single passes (two exchanges) in
    kernel modes 0 and 2 -- except the two-vector ATx of an EMPTY shard, which counts one pass in every mode;
  * n_allreduce counts exchanges (not messages: w_n | w_n2 travelling as one message is still one), only on a multi-rank context,
    only under set_timing 1 (at the call site) or 2 (through the event pairs); the overlapped exchange never touches it;
  * the kernel event pairs (set_timing 2) bracket one streaming launch per pass; the overlapped path and an empty shard record none.
"""
import os
import threading
import time

import numpy as np
import pytest

from gvamp_amd import capi, synth

pytestmark = pytest.mark.gpu

N, M = 1003, 517                 # ragged in both dimensions
TAU, GAM2, CG_STEPS = 2.0, 1.35, 3
CTR = ("n_ax", "n_ax_pass", "n_atx", "n_atx_pass", "n_allreduce", "n_ax_kernel", "n_atx_kernel")
SEQUENCE = ("ax", "atx", "ax2", "atx2", "lmmse", "cg2")
# multi-rank context, set_timing 2 (every column live).  Other settings of the same run: n_allreduce is 0 on a one-rank context
# and under set_timing 0; the two kernel columns are 0 unless set_timing is 2 (_expected).
ONE_PASS = [(1, 1, 0, 0, 1, 1, 0), (1, 1, 1, 1, 1, 1, 1), (3, 2, 1, 1, 2, 2, 1), (3, 2, 3, 2, 2, 2, 2), (4, 3, 4, 3, 3, 3, 3),
            (10, 6, 10, 6, 6, 6, 6)]
TWO_PASS = [(1, 1, 0, 0, 1, 1, 0), (1, 1, 1, 1, 1, 1, 1), (3, 3, 1, 1, 3, 3, 1), (3, 3, 3, 3, 3, 3, 3), (4, 4, 4, 4, 4, 4, 4),
            (10, 10, 10, 10, 10, 10, 10)]
# the empty rank of a two-rank job, first four calls of SEQUENCE: no kernel, the same exchanges as its peer
EMPTY_ONE_PASS = [(1, 1, 0, 0, 1, 0, 0), (1, 1, 1, 1, 1, 0, 0), (3, 2, 1, 1, 2, 0, 0), (3, 2, 3, 2, 2, 0, 0)]
EMPTY_TWO_PASS = [(1, 1, 0, 0, 1, 0, 0), (1, 1, 1, 1, 1, 0, 0), (3, 3, 1, 1, 3, 0, 0), (3, 3, 3, 2, 3, 0, 0)]
# overlapped exchange (kernel mode 1, multi-rank): ax, ax2, atx -- no all-reduce counted, no event pair around the chunked Ax
OVERLAP = [(1, 1, 0, 0, 0, 0, 0), (3, 2, 0, 0, 0, 0, 0), (3, 2, 1, 1, 0, 0, 1)]


def _expected(table, multi, timing):
    return [t[:4] + (t[4] if multi and timing else 0,) + (t[5:] if timing == 2 else (0, 0)) for t in table]


def _ctr(sh):
    c = sh.counters()
    return tuple(int(c[k]) for k in CTR)


class _host_cg:
    """the host-driven CG loops: their operator is lmmse_device / lmmse2_device, i.e. the dispatchers with the context's own
    w_n | w_n2 as outputs and the (addx, tau, gam2) epilogue"""

    def __enter__(self):
        os.environ["GV_CG_DEVICE"] = "0"

    def __exit__(self, *a):
        os.environ.pop("GV_CG_DEVICE", None)


def _mask(sh, n):
    present = np.ones(n, dtype=bool)
    present[5::11] = False
    m4 = np.zeros((n + 3) // 4, dtype=np.uint8)
    for i in np.nonzero(present)[0]:
        m4[i >> 2] |= 1 << (i & 3)
    sh.set_mask(m4, int(present.sum()))


def _geno(n, m, layout, mode, bed, **kw):
    sh = capi.Shard(n, m, anchor=(layout == "raw"), **kw)
    if layout != "raw":
        sh.set_layout(False, {"stripes": 1, "tile": 2}[layout])
    sh.set_kernel_mode(mode)
    sh.upload_bed(bed)
    _mask(sh, n)
    sh.compute_markers_statistics()
    return sh


def _operands(m):
    rng = np.random.default_rng(m + 1)
    return rng.standard_normal(m), np.sign(rng.standard_normal(m)) / np.sqrt(max(m, 1))


def _run(sh, x, x2, timing, steps=SEQUENCE):
    """the calls of `steps` in order -> (counters after each call, outputs), then the single-vector twins of the two-vector calls"""
    sh.set_timing(timing)
    sh.counters(reset=True)
    seen, out = [], {}
    z, z2, za, zb = (sh.vecN() for _ in range(4))
    w, w2, wa, wb, lm, mu_a, mu_b, m1, m2 = (sh.vecM() for _ in range(9))
    for name in steps:
        if name == "ax":
            sh.ax_dev(x, z)
        elif name == "atx":
            sh.atx_dev(z, w)
        elif name == "ax2":
            sh.ax2_dev(x, x2, za, zb)
        elif name == "atx2":
            sh.atx2_dev(za, zb, wa, wb)
        elif name == "lmmse":
            sh.lmmse_mult(x, TAU, GAM2, lm)
        else:
            with _host_cg():
                sh.cg_solve2(x, None, x2, TAU, GAM2, CG_STEPS, mu_a, mu_b)
        seen.append(_ctr(sh))
    sh.ax_dev(x2, z2)
    sh.atx_dev(z2, w2)
    if "cg2" in steps:
        with _host_cg():
            sh.cg_solve(x, None, TAU, GAM2, 1, CG_STEPS, m1)
            sh.cg_solve(x2, None, TAU, GAM2, 0, CG_STEPS, m2)
    names = ("z", "z2", "za", "zb", "w", "w2", "wa", "wb", "lm", "mu_a", "mu_b", "m1", "m2")
    vecs = (z, z2, za, zb, w, w2, wa, wb, lm, mu_a, mu_b, m1, m2)
    out = {k: v.download() for k, v in zip(names, vecs)}
    for v in vecs:
        v.free()
    return seen, out


TWINS = (("za", "z"), ("zb", "z2"), ("wa", "w"), ("wb", "w2"), ("mu_a", "m1"), ("mu_b", "m2"))


def _check_two_equal_one(out, what, pairs=TWINS):
    for two, one in pairs:
        assert not np.isnan(out[two]).any(), (what, two)
        assert np.any(out[two] != 0), (what, two)
        assert np.array_equal(out[two], out[one]), "%s: %s (two-vector) differs from %s (one-vector)" % (what, two, one)


def _check_tables(sh, x, x2, table):
    """one-rank and forced multi-rank runs under set_timing 0, 1, 2: counters against the literals, outputs against the first run"""
    bad, base = [], None
    for multi in (0, 1):
        sh.force_multi(multi)
        for timing in (0, 1, 2):
            seen, out = _run(sh, x, x2, timing)
            want = _expected(table, multi, timing)
            for name, got, exp in zip(SEQUENCE, seen, want):
                print("multi %d timing %d after %-5s: %s  (recorded %s)" % (multi, timing, name, got, exp))
                if got != exp:
                    bad.append((multi, timing, name, got, exp))
            what = "multi %d timing %d" % (multi, timing)
            _check_two_equal_one(out, what)
            if base is None:
                base = out
            for k in base:
                assert np.array_equal(base[k], out[k]), "%s: %s differs from the plain one-rank run" % (what, k)
    sh.force_multi(0)
    sh.set_timing(0)
    assert not bad, bad


@pytest.mark.parametrize("layout,mode", [("stripes", 1), ("stripes", 2), ("tile", 1), ("tile", 2), ("raw", 0), ("raw", 1), ("raw", 2)])
def test_genotype_dispatch_counters_and_two_vector_bits(layout, mode):
    bed = synth.synth_bed(N, M, seed=5, miss_ppm=8000)
    x, x2 = _operands(M)
    with _geno(N, M, layout, mode, bed) as sh:
        _check_tables(sh, sh.vecM(x), sh.vecM(x2), ONE_PASS if mode == 1 else TWO_PASS)


def test_methylation_dispatch_counters_and_two_vector_bits():
    x, x2 = _operands(M)
    with capi.Shard(N, M) as sh:
        sh.synth_meth(11)
        _mask(sh, N)
        sh.compute_markers_statistics()
        _check_tables(sh, sh.vecM(x), sh.vecM(x2), ONE_PASS)


@pytest.mark.parametrize("layout", ["stripes", "tile"])
def test_overlapped_exchange_counters_and_bits(layout):
    n = 2500                        # three units of 1024 individuals
    bed = synth.synth_bed(n, M, seed=6, miss_ppm=8000)
    xh, x2h = _operands(M)
    steps = ("ax", "ax2", "atx")
    with _geno(n, M, layout, 1, bed) as sh:
        x, x2 = sh.vecM(xh), sh.vecM(x2h)
        sh.force_multi(1)
        _, base = _run(sh, x, x2, 0, steps)
        bad = []
        for tiles in (2, 3):
            sh.set_overlap(tiles)
            for timing in (0, 1, 2):
                seen, out = _run(sh, x, x2, timing, steps)
                ms = sh.counters()["ms_allreduce"]
                for name, got, exp in zip(steps, seen, OVERLAP):
                    exp = exp[:5] + (exp[5:] if timing == 2 else (0, 0))
                    print("tiles %d timing %d after %-4s: %s  (recorded %s)" % (tiles, timing, name, got, exp))
                    if got != exp:
                        bad.append((tiles, timing, name, got, exp))
                what = "tiles %d timing %d" % (tiles, timing)
                assert ms == 0.0, (what, "ms_allreduce", ms)
                _check_two_equal_one(out, what, TWINS[:2])
                for k in ("z", "za", "zb", "w"):
                    assert np.array_equal(base[k], out[k]), "%s: %s differs from the undivided pass" % (what, k)
            sh.set_overlap(0)
        assert not bad, bad


@pytest.mark.parametrize("layout,mode", [("stripes", 1), ("stripes", 2), ("raw", 0)])
def test_empty_shard_takes_the_exchanges_of_its_peer(layout, mode):
    bed = synth.synth_bed(N, M, seed=7, miss_ppm=8000)
    xh, x2h = _operands(M)
    steps = SEQUENCE[:4]
    res, errors = [None, None], []

    def work(rank):
        try:
            m, s = (M, 0) if rank == 0 else (0, M)
            with _geno(N, m, layout, mode, bed if rank == 0 else np.zeros(0, dtype=np.uint8), Mt=M, S=s) as sh:
                sh.comm_init_local(8800 + 10 * mode + len(layout), 2, rank)
                x, x2 = sh.vecM(xh[s:s + m]), sh.vecM(x2h[s:s + m])
                res[rank] = [_run(sh, x, x2, timing, steps) for timing in (0, 1, 2)]
        except Exception as e:   # noqa: BLE001
            errors.append((rank, repr(e)))

    th = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(2)]
    for t in th:
        t.start()
    t_end = time.time() + 60
    for t in th:
        t.join(timeout=max(0.1, t_end - time.time()))
    assert not errors, errors                      # a rank that failed leaves its peer waiting: report the cause first
    assert not any(t.is_alive() for t in th), "a rank is stuck in a collective"
    bad = []
    for ti, timing in enumerate((0, 1, 2)):
        for rank, table in ((0, ONE_PASS if mode == 1 else TWO_PASS), (1, EMPTY_ONE_PASS if mode == 1 else EMPTY_TWO_PASS)):
            seen, out = res[rank][ti]
            for name, got, exp in zip(steps, seen, _expected(table, 1, timing)):
                print("rank %d timing %d after %-4s: %s  (recorded %s)" % (rank, timing, name, got, exp))
                if got != exp:
                    bad.append((rank, timing, name, got, exp))
        full, empty = res[0][ti][1], res[1][ti][1]
        for k in ("z", "z2", "za", "zb"):
            assert np.array_equal(full[k], empty[k]), "timing %d: %s differs between the ranks" % (timing, k)
        assert np.array_equal(full["za"], full["z"]) and np.array_equal(full["zb"], full["z2"]) and np.any(full["z"] != 0)
        assert np.array_equal(full["wa"], full["w"]) and np.array_equal(full["wb"], full["w2"])
        assert empty["w"].size == 0 and empty["wb"].size == 0
    assert not bad, bad
