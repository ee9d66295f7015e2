"""DevBuf / HostPinned (csrc/ins_devbuf.h) on the host, no GPU: tests/devbuf_host.cpp defines the allocation seam over malloc / free and checks the null
state, the moves, reset, ensure, the filled forms and that a handle whose N-th allocation fails holds nothing once it is destroyed.  It is compiled with
the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer and run as a program of its own."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "incompressiblenavierstokes.jl_amd", "csrc")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
# the sanitizer runtimes are linked statically: the program then does not depend on where a shared runtime would come in the process's library list
STATIC = {"g++": ["-static-libasan", "-static-libubsan"], "c++": ["-static-libasan", "-static-libubsan"], "clang++": ["-static-libsan"]}


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if cxx and shutil.which(cxx):
            return cxx
    return None


def test_ins_devbuf_header_needs_no_hip_header():
    includes = [ln for ln in open(os.path.join(CSRC, "ins_devbuf.h")) if ln.lstrip().startswith("#include")]
    assert includes and not [ln for ln in includes if "hip/" in ln or "ins_internal" in ln]


def test_devbuf_semantics_under_sanitizers(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = SANITIZE + STATIC.get(os.path.basename(cxx), [])
    r = subprocess.run([cxx, *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(tmp_path / "probe")]).returncode != 0:
        pytest.skip("the host compiler %s has no address / undefined-behaviour sanitizer runtime: %s" % (cxx, r.stderr.strip()[-200:]))
    exe = tmp_path / "devbuf_host"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC, "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "devbuf_host.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
