"""The library's host-side threaded code without a GPU and under the sanitizers ("Host-side threads under the sanitizers").

Four stand-alone programs under tests/host_threads/, each with its own main and a watchdog, include only the HIP-free header they test:

  copy_pool_main    gvamp_amd/csrc/gv_copy_pool.h    CopyPool, the helpers of every host copy of to_host / to_device: one run per
                                                     GV_XFER_THREADS in 0, 1, 3, 15
  read_slab_main    gvamp_amd/csrc/gv_read_slab.h    read_slab, the concurrent pread streams of the file ingest
  local_group_main  gvamp_amd/csrc/gv_local_group.h  LocalGroup, the in-process rank group the thread-per-rank GPU tests stand on
  shm_comm_main     gvamp_amd/csrc/host/shm_comm.cpp the process-shared transport behind GVAMP_COMM=host (linked in)

Every program is compiled here three ways -- plain (-O2), address + undefined (-O1 -g -fsanitize=address,undefined
-fno-sanitize-recover=all) and thread (-O1 -g -fsanitize=thread) -- and each binary runs on its own as a child process: exit
status 0 and nothing on stderr.  Nothing is loaded into Python.

shm_comm_main has no thread build.  The thread sanitizer keys its state on the virtual addresses of ONE process: what another
process, or another mapping of the segment, does to the shared slots is invisible to it, so such a run would prove nothing.  The
fork case of copy_pool_main runs in the plain and address builds only (a fork from a threaded process under the thread sanitizer is
that sanitizer's own business).

The thread build needs a runtime that can start on the host's kernel: a one-line program built with -fsanitize=thread is run first,
and only if THAT cannot start do the thread-build tests skip, with its stderr as the reason.

The watchdogs (alarm() in the programs) and the time limits here are hang detectors, not measurements: each is set at 20 times or
more what the thread build, the slowest, of that program takes (the measured times are in DESIGN.md), and each limit here lies
above the program's own watchdog, so that a hang is reported by the program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_threads")
CSRC = os.path.join(ROOT, "gvamp_amd", "csrc")

BUILDS = {
    "plain": ["-O2"],
    "address": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
    "thread": ["-O1", "-g", "-fsanitize=thread"],
}
# program -> (further sources, builds, seconds: above the program's own watchdog, so that a hang is reported by the program)
PROGRAMS = {
    "copy_pool_main": ([], ("plain", "address", "thread"), 960),
    "read_slab_main": ([], ("plain", "address", "thread"), 330),
    "local_group_main": ([], ("plain", "address", "thread"), 630),
    "shm_comm_main": ([os.path.join(CSRC, "host", "shm_comm.cpp")], ("plain", "address"), 150),
}
CASES = [(p, b) for p, (_, builds, _) in PROGRAMS.items() for b in builds]


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """every program in every build of its own, compiled side by side; the thread sanitizer's probe"""
    d = tmp_path_factory.mktemp("host_threads")
    (d / "probe.cpp").write_text("int main() { return 0; }\n")
    jobs = [("probe", subprocess.Popen(["g++", "-fsanitize=thread", "-o", str(d / "probe"), str(d / "probe.cpp")],
                                       stderr=subprocess.PIPE, text=True))]
    for prog, build in CASES:
        cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-pthread"] + BUILDS[build] + ["-I", CSRC, "-o", str(d / ("%s_%s" % (prog, build))),
                                                                                     os.path.join(SRC, prog + ".cpp")] + PROGRAMS[prog][0] + ["-lrt"]
        jobs.append(("%s (%s)" % (prog, build), subprocess.Popen(cmd, stderr=subprocess.PIPE, text=True)))
    for what, p in jobs:
        err = p.communicate()[1]
        assert p.returncode == 0, "%s does not compile:\n%s" % (what, err[-3000:])
    probe = subprocess.run([str(d / "probe")], capture_output=True, text=True, timeout=60)
    return d, (None if probe.returncode == 0 else "the thread sanitizer's runtime cannot start here: " + probe.stderr.strip()[-600:])


def _run(exe, args, env, seconds):
    res = subprocess.run([str(exe)] + args, env=dict(os.environ, **env), capture_output=True, text=True, timeout=seconds)
    assert res.returncode == 0, "%s %s %s: exit status %d\n%s" % (os.path.basename(str(exe)), args, env, res.returncode, res.stderr[-3000:])
    assert res.stderr.strip() == "", res.stderr[-3000:]          # a sanitizer reports on stderr


@pytest.mark.parametrize("prog,build", CASES, ids=["%s-%s" % c for c in CASES])
def test_program_runs_clean(built, prog, build):
    d, no_tsan = built
    if build == "thread" and no_tsan:
        pytest.skip(no_tsan)
    exe, seconds = d / ("%s_%s" % (prog, build)), PROGRAMS[prog][2]
    if prog == "copy_pool_main":
        for helpers in (0, 1, 3, 15):                              # the pool reads the variable once: one process each
            _run(exe, [] if build == "thread" else ["--fork"], {"GV_XFER_THREADS": str(helpers)}, seconds)
    else:
        _run(exe, [], {}, seconds)


def test_the_library_is_built_from_the_headers_under_test():
    """the .hip files include the three headers and no longer hold a copy of what moved; the headers include nothing of HIP"""
    def txt(name):
        return open(os.path.join(CSRC, name)).read()
    for hip, header, moved in (("gv_xfer.hip", "gv_copy_pool.h", "class CopyPool"), ("gv_ingest.hip", "gv_read_slab.h", "int read_slab("),
                               ("gv_comm.hip", "gv_local_group.h", "struct LocalGroup")):
        assert '#include "%s"' % header in txt(hip) and moved not in txt(hip) and moved in txt(header)
        assert "hip/" not in txt(header) and "gv_internal.h" not in txt(header)
