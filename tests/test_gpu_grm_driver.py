"""gvamp_main_real --run-mode grm on the simulated pedigree of tests/king_restatement.py written to a temporary
.bed.  With --grm-cutoff: <out>.grm.sp parsed back equals capi's grm_pairs, diagonal first, the values bit for bit through %.17g, with
and without --grm-marker-file.  Without: <out>.grm.bin / <out>.grm.N.bin hold the lower triangle of capi's grm_block rounded to float32.
No phenotype file is needed; the FATAL paths name their reason and leave no file."""
import os
import subprocess

import numpy as np
import pytest

import grm_restatement as gr
import king_restatement as kr
from gvamp_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "gvamp_amd", "gvamp_main_real")


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("GV_TUNE_CACHE", "0")
    for k in ("GVAMP_RESIDENT_LAYOUT", "RANK", "WORLD_SIZE"):
        monkeypatch.delenv(k, raising=False)


def _run(args, **kw):
    return subprocess.run([EXE, "--run-mode", "grm"] + args, capture_output=True, text=True, timeout=300, **kw)


def _parse_sp(path):
    rows = [ln.split() for ln in open(path).read().splitlines()]
    assert all(len(r) == 3 for r in rows)
    return (np.array([int(r[0]) for r in rows]), np.array([int(r[1]) for r in rows]), np.array([float(r[2]) for r in rows]))


@pytest.fixture(scope="module")
def ped(tmp_path_factory):
    cs = gr.case("pedigree")
    d = tmp_path_factory.mktemp("grm")
    bed = str(d / "ped.bed")
    with open(bed, "wb") as f:
        f.write(bytes([0x6C, 0x1B, 0x01]))
        f.write(cs["bed"].tobytes())
    use = (np.arange(cs["M"]) % 5 != 2).astype(np.uint8)
    use[61:67] = 0
    mfile = str(d / "use.bin")
    use.tofile(mfile)
    out = str(d) + "/"
    base = ["--bed-file", bed, "--N", str(cs["N"]), "--Mt", str(cs["M"]), "--out-dir", out]
    return cs, use, mfile, out, base


def test_the_sparse_file_equals_the_binding_and_the_fatal_paths_name_their_reason(ped):
    cs, use, mfile, out, base = ped
    N, M = cs["N"], cs["M"]
    with capi.Shard(N, M, device=0) as sh:
        sh.set_layout(False, 2)
        sh.upload_bed(cs["bed"])
        want = {"all": sh.grm_pairs(0.1), "sel": sh.grm_pairs(0.3, use=use)}
    for name, extra in (("all", ["--grm-cutoff", "0.1"]), ("sel", ["--grm-cutoff", "0.3", "--grm-marker-file", mfile])):
        res = _run(base + ["--out-name", name] + extra)
        assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
        i, j, v = _parse_sp(out + name + ".grm.sp")
        w = want[name]
        n = len(w[0])
        assert n > 0 and len(i) == N + n
        assert np.array_equal(i[:N], np.arange(N)) and np.array_equal(j[:N], np.arange(N)) and kr.same_bits(v[:N], w[4])      # the diagonal
        assert np.array_equal(i[N:], w[0]) and np.array_equal(j[N:], w[1]) and kr.same_bits(v[N:], w[2])
        line = [ln for ln in res.stdout.splitlines() if ln.startswith("grm: ")]
        assert len(line) == 1 and "%d pairs" % n in line[0] and "seconds" in line[0] and " counting of %d markers" % M in line[0], res.stdout[-2000:]
    truth = cs["truth"][want["all"][0], want["all"][1]]
    assert len(truth) == 83 and np.all(truth != kr.UNREL)                 # exactly the related pairs of the pedigree
    # the FATAL paths
    res = _run(base + ["--out-name", "bad", "--geno-format", "dosage8"])
    assert res.returncode != 0 and "FATAL: --run-mode grm works on 2-bit genotypes only" in res.stdout, res.stdout[-2000:]
    res = _run(base + ["--out-name", "bad"], env=dict(os.environ, RANK="0", WORLD_SIZE="2"))
    assert res.returncode != 0 and "FATAL: --run-mode grm runs on one rank" in res.stdout, res.stdout[-2000:]
    short = out + "short.bin"
    use[:10].tofile(short)
    res = _run(base + ["--out-name", "bad", "--grm-marker-file", short])
    assert res.returncode != 0 and "FATAL: --grm-marker-file" in res.stdout and "must hold Mt = %d bytes" % M in res.stdout, res.stdout[-2000:]
    res = _run(base + ["--out-name", "bad", "--grm-cutoff", "nan"])
    assert res.returncode != 0 and "FATAL: gv_grm_pairs" in res.stdout and "cutoff" in res.stdout, res.stdout[-2000:]
    for extra in (["--grm-cutoff", "0.1"], []):
        res = _run(base + ["--out-name", "bad", "--resident-layout", "1"] + extra)
        assert res.returncode != 0 and "two stripe sets" in res.stdout and "tile layout" in res.stdout, res.stdout[-2000:]
    assert not any(f.startswith("bad") for f in os.listdir(out))


def test_the_dense_files_hold_the_lower_triangle_of_the_binding_as_float32(ped):
    cs, use, mfile, out, base = ped
    N, M = cs["N"], cs["M"]
    with capi.Shard(N, M, device=0) as sh:
        sh.set_layout(False, 2)
        sh.upload_bed(cs["bed"])
        want = {"dense": sh.grm_block(0, N, 0, N), "densesel": sh.grm_block(0, N, 0, N, use=use)}
    il, jl = np.tril_indices(N)                     # row by row, j <= i
    for name, extra in (("dense", []), ("densesel", ["--grm-marker-file", mfile])):
        res = _run(base + ["--out-name", name] + extra)
        assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
        a = np.fromfile(out + name + ".grm.bin", dtype=np.float32)
        m = np.fromfile(out + name + ".grm.N.bin", dtype=np.float32)
        wa, wm = want[name]
        assert a.shape == m.shape == (N * (N + 1) // 2,)
        assert np.array_equal(a.view(np.uint32), wa[il, jl].astype(np.float32).view(np.uint32))
        assert np.array_equal(m, wm[il, jl].astype(np.float32))
        line = [ln for ln in res.stdout.splitlines() if ln.startswith("grm: ")]
        assert len(line) == 1 and "%d pairs" % (N * (N + 1) // 2) in line[0] and "seconds" in line[0], res.stdout[-2000:]
