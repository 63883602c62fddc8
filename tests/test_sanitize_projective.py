"""CPU: the projective refinement's host code under sanitizers.  csrc/projective_solve.cpp + csrc/host_io.cpp are compiled directly with
g++ -fsanitize=address,undefined and, separately, -fsanitize=thread, together with the stand-alone tests/cxx/projective_sanitize.cpp (its own
main; a survey whose factorisation takes a team of threads), and run.  The probe, the skip rules and the setarch handling are
tests/test_sanitize.py's.  Nothing is loaded into Python under a sanitizer."""
import os
import subprocess

import pytest

from tests.test_sanitize import CSRC, ROOT, _runner


def _build_and_run(tmp_path, flags, tag):
    prefix = _runner(tmp_path, flags, tag)
    exe = str(tmp_path / ("projective_sanitize_" + tag))
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-pthread"] + flags + [
        "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cxx", "projective_sanitize.cpp"),
        os.path.join(CSRC, "projective_solve.cpp"), os.path.join(CSRC, "host_io.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("cannot find" in r.stderr or "unrecognized" in r.stderr):
        pytest.skip("sanitizer runtime not installed: " + r.stderr[-300:])
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1",
               MI355_HOST_THREADS="4")
    r = subprocess.run(prefix + [exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "SANITIZE_OK" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])


def test_projective_host_code_under_asan_ubsan(tmp_path):
    _build_and_run(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "asan")


def test_projective_host_code_under_tsan(tmp_path):
    _build_and_run(tmp_path, ["-fsanitize=thread"], "tsan")
