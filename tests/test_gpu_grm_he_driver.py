"""gvamp_main_real --run-mode he on the simulated pedigree of tests/king_restatement.py written to a temporary
.bed, with two phenotype files (one with NA lines) and a marker file: <out>.HEreg parsed back equals capi's grm_he, the values bit
for bit through %.17g; the FATAL paths name their reason and leave no file."""
import os
import subprocess

import numpy as np
import pytest

import grm_he_restatement as hr
import grm_restatement as gr
import king_restatement as kr
from gvamp_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "gvamp_amd", "gvamp_main_real")


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("GV_TUNE_CACHE", "0")
    for k in ("GVAMP_RESIDENT_LAYOUT", "RANK", "WORLD_SIZE", "GV_GRM_PART_MB"):
        monkeypatch.delenv(k, raising=False)


def _run(args, **kw):
    return subprocess.run([EXE, "--run-mode", "he"] + args, capture_output=True, text=True, timeout=300, **kw)


def test_the_hereg_file_equals_the_binding_and_the_fatal_paths_name_their_reason(tmp_path):
    cs = gr.case("pedigree")
    N, M = cs["N"], cs["M"]
    bed = str(tmp_path / "ped.bed")
    with open(bed, "wb") as f:
        f.write(bytes([0x6C, 0x1B, 0x01]))
        f.write(cs["bed"].tobytes())
    use = (np.arange(M) % 5 != 2).astype(np.uint8)
    use[61:67] = 0
    mfile = str(tmp_path / "use.bin")
    use.tofile(mfile)
    Y = hr.traits(cs, 55, n=2)
    files = []
    for c in range(2):
        files.append(str(tmp_path / ("y%d.phen" % c)))
        with open(files[-1], "w") as f:
            for n in range(N):
                f.write("f%d i%d %s\n" % (n, n, "NA" if np.isnan(Y[n, c]) else repr(float(Y[n, c]))))
    out = str(tmp_path) + "/"
    base = ["--bed-file", bed, "--N", str(N), "--Mt", str(M), "--out-dir", out, "--phen-files", ",".join(files)]
    with capi.Shard(N, M, device=0) as sh:
        sh.set_layout(False, 2)
        sh.upload_bed(cs["bed"])
        want = {"all": sh.grm_he(Y), "sel": sh.grm_he(Y, use=use)}
    assert np.isnan(Y[:, 1]).sum() > 0 and not np.array_equal(want["all"]["h2"], want["sel"]["h2"])
    for name, extra in (("all", []), ("sel", ["--grm-marker-file", mfile])):
        res = _run(base + ["--out-name", name] + extra)
        assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
        lines = open(out + name + ".HEreg").read().splitlines()
        assert lines[0].split() == ["trait", "n_ind", "n_pairs", "mean_a", "var_a", "h2", "intercept", "se_ols", "se_jack"] and len(lines) == 3
        for c in range(2):
            tok = lines[1 + c].split()
            w = want[name][c]
            assert tok[0] == files[c] and int(tok[1]) == w["n_ind"] and int(tok[2]) == w["n_pairs"] and len(tok) == 9
            mean = w["sum_a"] / float(w["n_pairs"])
            var = w["sum_aa"] / float(w["n_pairs"]) - mean * mean
            assert kr.same_bits(np.array([float(t) for t in tok[3:4] + tok[5:]]),
                                np.array([mean, w["h2"], w["intercept"], w["se_ols"], w["se_jack"]])), (name, c, tok)
            # var_a = sum_aa / n - mean^2, three roundings or two with a fused multiply-add: the host compiler's choice
            assert abs(float(tok[4]) - var) <= 4 * 2.0 ** -53 * (w["sum_aa"] / float(w["n_pairs"]) + mean * mean), (name, c, tok)
        line = [ln for ln in res.stdout.splitlines() if ln.startswith("he: ")]
        assert len(line) == 1 and "seconds" in line[0] and "2 traits" in line[0] and "1 passes" in line[0], res.stdout[-2000:]
        assert " counting of %d markers" % M in line[0] and "%d blocks" % 3 in line[0]
    # the FATAL paths
    res = _run(base + ["--out-name", "bad", "--geno-format", "dosage8"])
    assert res.returncode != 0 and "FATAL: --run-mode he works on 2-bit genotypes only" in res.stdout, res.stdout[-2000:]
    res = _run(base + ["--out-name", "bad"], env=dict(os.environ, RANK="0", WORLD_SIZE="2"))
    assert res.returncode != 0 and "FATAL: --run-mode he runs on one rank" in res.stdout, res.stdout[-2000:]
    res = _run(base[:-1] + [files[0] + "," + out + "nothing.phen", "--out-name", "bad"])
    assert res.returncode != 0 and "FATAL" in res.stdout + res.stderr and "nothing.phen not found" in res.stdout + res.stderr
    short = out + "short.bin"
    use[:10].tofile(short)
    res = _run(base + ["--out-name", "bad", "--grm-marker-file", short])
    assert res.returncode != 0 and "FATAL: --grm-marker-file" in res.stdout and "must hold Mt = %d bytes" % M in res.stdout, res.stdout[-2000:]
    res = _run(base + ["--out-name", "bad", "--resident-layout", "1"])
    assert res.returncode != 0 and "FATAL: gv_grm_he" in res.stdout and "two stripe sets" in res.stdout, res.stdout[-2000:]
    inf = out + "inf.phen"
    with open(inf, "w") as f:
        for n in range(N):
            f.write("f%d i%d %s\n" % (n, n, "inf" if n == 4 else "0.5"))
    res = _run(base[:-1] + [inf, "--out-name", "bad"])
    assert res.returncode != 0 and "FATAL: gv_grm_he" in res.stdout and "infinite" in res.stdout, res.stdout[-2000:]
    assert not any(f.startswith("bad") for f in os.listdir(out))
