"""What gvamp_main_real and gvamp_main_real_probit refuse before any device work (no GPU): a table of bad command lines, each held to
its exit status and to EVERYTHING the driver prints on stdout after the echoed option block, byte for byte.  divide_work's
"INFO   : rank ..." line is part of that text, so a case also pins whether its refusal comes before or after the shard is computed.
The expected text is at the end of the file; {tmp} stands for the directory of the case's input files."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = {"real": os.path.join(ROOT, "gvamp_amd", "gvamp_main_real"), "probit": os.path.join(ROOT, "gvamp_amd", "gvamp_main_real_probit")}
B = ["--bed-file", "x.bed", "--N", "8", "--Mt", "12"]
BT = ["--bed-file-test", "x.bed", "--N-test", "8", "--Mt-test", "12"]
P12 = ["--clump-p-file", "{tmp}/f64x12.bin"]


def write_inputs(d):
    """the input files of the cases: phenotype files of 8 lines, raw float64 files for 12 markers, and their broken variants"""
    def text(name, lines):
        with open(os.path.join(d, name), "w") as f:
            f.write("".join(l + "\n" for l in lines))
    text("a.phen", ["f%d i%d %d.5" % (n, n, n) for n in range(8)])
    text("b.phen", ["f%d i%d %d" % (n, n, (n * 5) % 7) for n in range(8)])
    text("two_tokens.phen", ["f%d i%d" % (n, n) for n in range(8)])
    text("one_line.phen", ["f0 i0 1.5"])
    text("all_na.phen", ["f%d i%d NA" % (n, n) for n in range(8)])
    for name, size in (("f64x12.bin", 96), ("bytes24.bin", 24), ("bytes5.bin", 5)):
        with open(os.path.join(d, name), "wb") as f:
            f.write(bytes(size))


# (id, driver, arguments, WORLD_SIZE or None)
CASES = [
    ("unknown_mode", "real", ["--run-mode", "nonsense"] + B, None),
    ("precond_ld_dosage16", "real", ["--run-mode", "infere", "--cg-precond", "ld", "--ld-dosage", "1", "--geno-format", "dosage16"] + B, None),
    ("infere_no_phen", "real", ["--run-mode", "infere"] + B, None),
    ("pvals_calc_no_phen", "real", ["--run-mode", "pvals-calc"] + B, None),
    ("pca_no_phen", "real", ["--run-mode", "pca", "--pca-k", "2"] + B, None),
    ("screen_no_phen", "real", ["--run-mode", "screen"] + B, None),
    ("ldscore_no_phen", "real", ["--run-mode", "ldscore"] + B, None),
    ("clump_no_phen", "real", ["--run-mode", "clump", "--ld-window", "3"] + P12 + B, None),
    ("test_no_phen_test", "real", ["--run-mode", "test"] + BT, None),
    ("both_no_phen_test", "real", ["--run-mode", "both", "--phen-files", "{tmp}/a.phen"] + B, None),
    ("ldscore_dosage8", "real", ["--run-mode", "ldscore", "--geno-format", "dosage8"] + B, None),
    ("ldscore_dosage16_ld_dosage", "real", ["--run-mode", "ldscore", "--geno-format", "dosage16", "--ld-dosage", "1"] + B, None),
    ("ldscore_two_ranks", "real", ["--run-mode", "ldscore"] + B, 2),
    ("ldscore_two_windows", "real", ["--run-mode", "ldscore", "--ld-window", "5", "--ld-wind-kb", "3"] + B, None),
    ("ldscore_kb_no_bim", "real", ["--run-mode", "ldscore", "--ld-wind-kb", "3"] + B, None),
    ("ldscore_cm_no_bim", "real", ["--run-mode", "ldscore", "--ld-wind-cm", "3"] + B, None),
    ("clump_dosage8", "real", ["--run-mode", "clump", "--geno-format", "dosage8"] + B, None),
    ("clump_two_ranks", "real", ["--run-mode", "clump"] + B, 2),
    ("clump_two_windows", "real", ["--run-mode", "clump", "--clump-kb", "5", "--ld-window", "3"] + B, None),
    ("clump_default_kb_no_bim", "real", ["--run-mode", "clump"] + P12 + B, None),
    ("clump_cm_no_bim", "real", ["--run-mode", "clump", "--ld-wind-cm", "1"] + B, None),
    ("clump_no_p_file", "real", ["--run-mode", "clump", "--ld-window", "3"] + B, None),
    ("clump_missing_p_file", "real", ["--run-mode", "clump", "--ld-window", "3", "--clump-p-file", "{tmp}/none.bin"] + B, None),
    ("clump_short_p_file", "real", ["--run-mode", "clump", "--ld-window", "3", "--clump-p-file", "{tmp}/bytes24.bin"] + B, None),
    ("score_no_score_file", "real", ["--run-mode", "score"] + BT, None),
    ("score_thresholds_alone", "real", ["--run-mode", "score", "--score-file", "{tmp}/f64x12.bin", "--score-p-thresholds", "0.1,0.5"] + BT, None),
    ("score_thresholds_five_cols", "real", ["--run-mode", "score", "--score-file", "{tmp}/f64x12.bin", "--score-p-thresholds", "0.1,0.5",
                                            "--score-p-file", "{tmp}/f64x12.bin", "--score-clump-index", "{tmp}/f64x12.bin", "--score-cols", "5"] + BT,
     None),
    ("score_missing_score_file", "real", ["--run-mode", "score", "--score-file", "{tmp}/none.bin"] + BT, None),
    ("score_short_score_file", "real", ["--run-mode", "score", "--score-file", "{tmp}/bytes24.bin"] + BT, None),
    ("screen_dosage8", "real", ["--run-mode", "screen", "--geno-format", "dosage8"] + B, None),
    ("screen_too_many_values", "real", ["--run-mode", "screen", "--phen-files", "{tmp}/a.phen,{tmp}/b.phen", "--bed-file", "x.bed", "--N", "8",
                                        "--Mt", "2147483647"], None),
    ("screen_two_tokens", "real", ["--run-mode", "screen", "--phen-files", "{tmp}/two_tokens.phen"] + B, None),
    ("screen_one_line", "real", ["--run-mode", "screen", "--phen-files", "{tmp}/one_line.phen"] + B, None),
    ("screen_all_na", "real", ["--run-mode", "screen", "--phen-files", "{tmp}/all_na.phen"] + B, None),
    ("pca_no_k", "real", ["--run-mode", "pca"] + B, None),
    ("pca_block_below_k", "real", ["--run-mode", "pca", "--pca-k", "4", "--pca-block", "3"] + B, None),
    ("pca_block_above_max", "real", ["--run-mode", "pca", "--pca-k", "4", "--pca-block", "33"] + B, None),
    ("pca_too_many_values", "real", ["--run-mode", "pca", "--pca-k", "2", "--bed-file", "x.bed", "--N", "8", "--Mt", "2147483647"], None),
    ("king_dosage8", "real", ["--run-mode", "king", "--geno-format", "dosage8"] + B, None),
    ("king_two_ranks", "real", ["--run-mode", "king"] + B, 2),
    ("king_short_marker_file", "real", ["--run-mode", "king", "--king-marker-file", "{tmp}/bytes5.bin"] + B, None),
    ("king_missing_marker_file", "real", ["--run-mode", "king", "--king-marker-file", "{tmp}/none.bin"] + B, None),
    ("probit_no_model", "probit", ["--run-mode", "infere"] + B, None),
    ("probit_predict", "probit", ["--model", "bin_class", "--run-mode", "predict"] + B, None),
    ("probit_infere_no_phen", "probit", ["--model", "bin_class", "--run-mode", "infere"] + B, None),
    ("probit_both_no_phen_test", "probit", ["--model", "bin_class", "--run-mode", "both", "--phen-files", "{tmp}/a.phen"] + B, None),
]


def run_case(case, d):
    """exit status and the text on stdout after the blank line that ends the echoed option block, with `d` written as {tmp}"""
    _id, driver, args, world = case
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    if world:
        env["WORLD_SIZE"] = str(world)
    r = subprocess.run([EXE[driver]] + [a.replace("{tmp}", d) for a in args], capture_output=True, text=True, env=env, cwd=d, timeout=60)
    head = "\nardyh command line options:\n"
    assert r.stdout.startswith(head), r.stdout
    end = r.stdout.index("\n\n", len(head)) + 2
    return r.returncode, r.stdout[end:].replace(d, "{tmp}")


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    import __graft_entry__ as g
    g.build()
    d = str(tmp_path_factory.mktemp("refusals"))
    write_inputs(d)
    return d


def test_every_case_has_its_expected_text():
    assert len(CASES) == len(EXPECTED) == len({c[0] for c in CASES}) and all(c[0] in EXPECTED for c in CASES)
    assert all(status == 1 and "FATAL" in text for status, text in EXPECTED.values())


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_driver_refuses_with_the_same_status_and_text(inputs, case):
    status, text = run_case(case, inputs)
    want_status, want_text = EXPECTED[case[0]]
    assert text == want_text
    assert status == want_status


# ---- expected text (of the drivers before their main() was split; generated once, then held) ----
EXPECTED = {'unknown_mode': (1, 'FATAL: unknown --run-mode "nonsense"\n'),
 'precond_ld_dosage16': (1, 'FATAL: --cg-precond ld with --ld-dosage 1 covers --geno-format dosage8 only, not --geno-format dosage16\n'),
 'infere_no_phen': (1,
                    'INFO   : rank    0 has 12 markers over tot Mt = 12, max Mm = 12, starting at S = 0\n'
                    'FATAL  : no phen file(s) provided! Please use the --phen-files option.\n'),
 'pvals_calc_no_phen': (1,
                        'INFO   : rank    0 has 12 markers over tot Mt = 12, max Mm = 12, starting at S = 0\n'
                        'FATAL  : no phen file(s) provided! Please use the --phen-files option.\n'),
 'pca_no_phen': (1,
                 'INFO   : rank    0 has 12 markers over tot Mt = 12, max Mm = 12, starting at S = 0\n'
                 'FATAL  : no phen file(s) provided! Please use the --phen-files option.\n'),
 'screen_no_phen': (1,
                    'INFO   : rank    0 has 12 markers over tot Mt = 12, max Mm = 12, starting at S = 0\n'
                    'FATAL  : no phen file(s) provided! Please use the --phen-files option.\n'),
 'ldscore_no_phen': (1, 'FATAL  : no phen file(s) provided! Please use the --phen-files option.\n'),
 'clump_no_phen': (1, 'FATAL  : no phen file(s) provided! Please use the --phen-files option.\n'),
 'test_no_phen_test': (1,
                       'INFO   : rank    0 has 12 markers over tot Mt = 12, max Mm = 12, starting at S = 0\n'
                       'FATAL  : no phen file(s) provided! Please use the --phen-files-test option.\n'),
 'both_no_phen_test': (1,
                       'INFO   : rank    0 has 12 markers over tot Mt = 12, max Mm = 12, starting at S = 0\n'
                       'FATAL  : no phen file(s) provided! Please use the --phen-files-test option.\n'),
 'ldscore_dosage8': (1, 'FATAL: --run-mode ldscore works on 2-bit genotypes only, not on --geno-format dosage8\n'),
 'ldscore_dosage16_ld_dosage': (1, 'FATAL: --run-mode ldscore works on 2-bit genotypes only, not on --geno-format dosage16\n'),
 'ldscore_two_ranks': (1,
                       "FATAL: --run-mode ldscore runs on one rank: the band stops at a shard's edges, so the scores of a sharded job would miss "
                       'their neighbours across them\n'),
 'ldscore_two_windows': (1, 'FATAL: exactly one of --ld-window, --ld-wind-kb and --ld-wind-cm may be given\n'),
 'ldscore_kb_no_bim': (1, 'FATAL: --ld-wind-kb needs --bim-file: the positions are its base-pair column\n'),
 'ldscore_cm_no_bim': (1, 'FATAL: --ld-wind-cm needs --bim-file: the positions are its cM column\n'),
 'clump_dosage8': (1, 'FATAL: --run-mode clump works on 2-bit genotypes only, not on --geno-format dosage8\n'),
 'clump_two_ranks': (1,
                     "FATAL: --run-mode clump runs on one rank: the band stops at a shard's edges, so the clumps of a sharded job would miss their "
                     'members across them\n'),
 'clump_two_windows': (1, 'FATAL: exactly one of --clump-kb, --ld-wind-cm and --ld-window may be given\n'),
 'clump_default_kb_no_bim': (1, 'FATAL: --clump-kb needs --bim-file: the positions are its base-pair column\n'),
 'clump_cm_no_bim': (1, 'FATAL: --ld-wind-cm needs --bim-file: the positions are its cM column\n'),
 'clump_no_p_file': (1, 'FATAL: --run-mode clump needs --clump-p-file: 12 raw float64 p-values, the format of <out>_assoc_p.bin\n'),
 'clump_missing_p_file': (1, 'FATAL: cannot open the p file {tmp}/none.bin\n'),
 'clump_short_p_file': (1, 'FATAL: the p file {tmp}/bytes24.bin holds 24 bytes, fewer than the 96 of 12 float64 values\n'),
 'score_no_score_file': (1, 'FATAL: --run-mode score needs --score-file: --score-cols x 12 raw float64 weights, column after column\n'),
 'score_thresholds_alone': (1, 'FATAL: --score-clump-index, --score-p-file and --score-p-thresholds go together: all three or none\n'),
 'score_thresholds_five_cols': (1,
                                'FATAL: --score-p-thresholds builds its columns from column 0 of the score file: it needs --score-cols 1, not 5\n'),
 'score_missing_score_file': (1, 'FATAL: cannot open the score file {tmp}/none.bin\n'),
 'score_short_score_file': (1, 'FATAL: the score file {tmp}/bytes24.bin holds 24 bytes, fewer than the 96 of 12 float64 values\n'),
 'screen_dosage8': (1, 'FATAL: --run-mode screen works on 2-bit genotypes only, not on --geno-format dosage8\n'),
 'screen_too_many_values': (1,
                            'INFO   : rank    0 has 2147483647 markers over tot Mt = 2147483647, max Mm = 2147483647, starting at S = 0\n'
                            'FATAL: --run-mode screen: 2 columns x 2147483647 markers exceed the 2^31 - 1 values of an output file\n'),
 'screen_two_tokens': (1,
                       'INFO   : rank    0 has 12 markers over tot Mt = 12, max Mm = 12, starting at S = 0\n'
                       'FATAL: phenotype line with fewer than 3 columns in {tmp}/two_tokens.phen\n'),
 'screen_one_line': (1,
                     'INFO   : rank    0 has 12 markers over tot Mt = 12, max Mm = 12, starting at S = 0\n'
                     'FATAL: {tmp}/one_line.phen holds 1 lines, not --N = 8\n'),
 'screen_all_na': (1,
                   'INFO   : rank    0 has 12 markers over tot Mt = 12, max Mm = 12, starting at S = 0\n'
                   'FATAL: --run-mode screen: 0 complete cases leave the test no degree of freedom\n'),
 'pca_no_k': (1, 'FATAL: --run-mode pca needs --pca-k K, the number of principal components (1..32)\n'),
 'pca_block_below_k': (1, 'FATAL: --run-mode pca: the block has to hold --pca-k = 4 vectors and at most 32 (--pca-block 3)\n'),
 'pca_block_above_max': (1, 'FATAL: --run-mode pca: the block has to hold --pca-k = 4 vectors and at most 32 (--pca-block 33)\n'),
 'pca_too_many_values': (1, 'FATAL: --run-mode pca: 2 columns x 2147483647 markers exceed the 2^31 - 1 values of an output file\n'),
 'king_dosage8': (1, 'FATAL: --run-mode king works on 2-bit genotypes only, not on --geno-format dosage8\n'),
 'king_two_ranks': (1,
                    'FATAL: --run-mode king runs on one rank: the counts of a pair are sums over the markers of all ranks, and the integer '
                    'all-reduce that would add them is not built\n'),
 'king_short_marker_file': (1, 'FATAL: --king-marker-file {tmp}/bytes5.bin must hold Mt = 12 bytes of 0 / 1 (5 bytes read)\n'),
 'king_missing_marker_file': (1, 'FATAL: --king-marker-file {tmp}/none.bin must hold Mt = 12 bytes of 0 / 1 (cannot open it)\n'),
 'probit_no_model': (1, 'FATAL: gvamp_main_real_probit needs --model bin_class\n'),
 'probit_predict': (1, 'FATAL: --run-mode predict is not a mode of main_real_probit (infere | test | both)\n'),
 'probit_infere_no_phen': (1,
                           'INFO   : rank    0 has 12 markers over tot Mt = 12, max Mm = 12, starting at S = 0\n'
                           'FATAL  : no phen file(s) provided! Please use the --phen-files option.\n'),
 'probit_both_no_phen_test': (1,
                              'INFO   : rank    0 has 12 markers over tot Mt = 12, max Mm = 12, starting at S = 0\n'
                              'FATAL  : no phen file(s) provided! Please use the --phen-files-test option.\n')}
