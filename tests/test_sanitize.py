"""CPU: the library's host-only translation units under sanitizers (the reference has none and carries known races).
csrc/host_io.cpp + csrc/overlap.cpp are compiled directly with g++ -fsanitize=address,undefined and, separately, -fsanitize=thread,
together with tests/cxx/host_sanitize.cpp, and run on the reference's committed artefacts.  (mi355_pair_schedule lives in api.hip
and needs HIP headers: a two-line stand-alone copy would not test the product, so the driver only calls it when linked in.)"""
import os
import platform
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "imagemosaicing_amd", "csrc")


def _runner(tmp_path, flags, tag):
    """how a program built with these flags is started here.  GCC 11's ThreadSanitizer runtime cannot place its shadow memory under the
    address-space randomisation of newer kernels (vm.mmap_rnd_bits above 28) and dies before main with no message; with randomisation
    off for that one process (setarch -R) it starts.  A probe program tells whether the runtime can start here at all."""
    prefix = [shutil.which("setarch"), platform.machine(), "-R"] if tag == "tsan" and shutil.which("setarch") else []
    probe = tmp_path / "probe.cpp"
    probe.write_text("#include <thread>\nint x;\nint main() { std::thread t([] { x = 1; }); t.join(); return x - 1; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-pthread"] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode != 0 and ("cannot find" in r.stderr or "unrecognized" in r.stderr):
        pytest.skip("sanitizer runtime not installed: " + r.stderr[-300:])
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run(prefix + [str(tmp_path / "probe")], capture_output=True, text=True, timeout=120)
    if r.returncode < 0:
        pytest.skip("the %s runtime cannot start on this machine: a two-line program dies with signal %d before main" % (tag, -r.returncode))
    return prefix


def _build_and_run(tmp_path, flags, tag):
    prefix = _runner(tmp_path, flags, tag)
    exe = str(tmp_path / ("host_sanitize_" + tag))
    # mi355_pair_schedule is defined in api.hip (HIP TU): give the driver the one symbol through a weak stub that reports "not linked"
    stub = tmp_path / "stub.cpp"
    stub.write_text('#include <cstdlib>\n#include "mi355_mosaic.h"\nextern "C" __attribute__((weak)) int mi355_pair_schedule(int, int, int, int, int32_t*, int, int* n) { *n = 33; return -1; }\n'
                    'extern "C" __attribute__((weak)) void mi355_free(void* p) { free(p); }\n')
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-pthread"] + flags + [
        "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cxx", "host_sanitize.cpp"),
        os.path.join(CSRC, "host_io.cpp"), os.path.join(CSRC, "overlap.cpp"), str(stub), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("cannot find" in r.stderr or "unrecognized" in r.stderr):
        pytest.skip("sanitizer runtime not installed: " + r.stderr[-300:])
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run(prefix + [exe, os.path.join(ROOT, "tests", "golden"), str(tmp_path)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "SANITIZE_OK" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])


def test_host_code_under_asan_ubsan(tmp_path):
    _build_and_run(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "asan")


def test_host_code_under_tsan(tmp_path):
    _build_and_run(tmp_path, ["-fsanitize=thread"], "tsan")
