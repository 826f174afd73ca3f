"""gvamp_main_real --run-mode king on the simulated pedigree of tests/king_restatement.py written to a temporary
.bed: <out>_king.kin0.txt parsed back equals capi's king_pairs (integers as integers, the kinship bit for bit through %.17g), with and
without --king-marker-file, and no phenotype file is needed; the FATAL paths name their reason."""
import os
import subprocess

import numpy as np
import pytest

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
    return subprocess.run([EXE, "--run-mode", "king"] + args, capture_output=True, text=True, timeout=300, **kw)


def _parse(path):
    rows = [ln.split() for ln in open(path).read().splitlines()]
    assert all(len(r) == 8 for r in rows)
    ints = np.array([[int(t) for t in r[:7]] for r in rows], dtype=np.int64).reshape(-1, 7)
    return ints[:, 0], ints[:, 1], np.array([float(r[7]) for r in rows]), ints[:, 2:7]


def test_the_pair_file_equals_the_binding_and_the_fatal_paths_name_their_reason(tmp_path):
    cs = kr.case("pedigree")
    N, M = cs["N"], cs["M"]
    bed = str(tmp_path / "ped.bed")
    with open(bed, "wb") as f:
        f.write(bytes([0x6C, 0x1B, 0x01]))
        f.write(cs["bed"].tobytes())
    use = (np.arange(M) % 5 != 2).astype(np.uint8)
    use[61:67] = 0
    mfile = str(tmp_path / "use.bin")
    use.tofile(mfile)
    out = str(tmp_path) + "/"
    base = ["--bed-file", bed, "--N", str(N), "--Mt", str(M), "--out-dir", out]
    with capi.Shard(N, M, device=0) as sh:
        sh.set_layout(False, 2)
        sh.upload_bed(cs["bed"])
        want = {"all": sh.king_pairs(kr.CUT_SECOND), "sel": sh.king_pairs(0.2, use=use)}
    for name, extra in (("all", ["--king-cutoff", str(kr.CUT_SECOND)]), ("sel", ["--king-cutoff", "0.2", "--king-marker-file", mfile])):
        res = _run(base + ["--out-name", name] + extra)
        assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
        i, j, kin, cnt = _parse(out + name + "_king.kin0.txt")
        w = want[name]
        assert len(w[0]) > 0 and np.array_equal(i, w[0]) and np.array_equal(j, w[1]) and np.array_equal(cnt, w[3])
        assert kr.same_bits(kin, w[2])
        line = [ln for ln in res.stdout.splitlines() if ln.startswith("king: ")]
        assert len(line) == 1 and "%d pairs" % len(i) in line[0] and "seconds" in line[0], res.stdout[-2000:]
    truth = cs["truth"][want["all"][0], want["all"][1]]
    assert len(truth) == 83 and np.all(truth != kr.UNREL)                 # exactly the related pairs of the pedigree
    # the FATAL paths
    res = _run(base + ["--out-name", "bad", "--geno-format", "dosage8"])
    assert res.returncode != 0 and "FATAL: --run-mode king works on 2-bit genotypes only" in res.stdout, res.stdout[-2000:]
    res = _run(base + ["--out-name", "bad"], env=dict(os.environ, RANK="0", WORLD_SIZE="2"))
    assert res.returncode != 0 and "FATAL: --run-mode king runs on one rank" in res.stdout, res.stdout[-2000:]
    short = str(tmp_path / "short.bin")
    use[:10].tofile(short)
    res = _run(base + ["--out-name", "bad", "--king-marker-file", short])
    assert res.returncode != 0 and "FATAL: --king-marker-file" in res.stdout and "must hold Mt = %d bytes" % M in res.stdout, res.stdout[-2000:]
    res = _run(base + ["--out-name", "bad", "--king-cutoff", "nan"])
    assert res.returncode != 0 and "FATAL: gv_king_pairs" in res.stdout and "cutoff" in res.stdout, res.stdout[-2000:]
    res = _run(base + ["--out-name", "bad", "--resident-layout", "1"])
    assert res.returncode != 0 and "two stripe sets" in res.stdout and "tile layout" in res.stdout, res.stdout[-2000:]
    assert not any(f.startswith("bad") for f in os.listdir(out))
