"""Device and pinned-host memory is allocated and freed in one translation unit (csrc/ins_devmem.hip, the seam under DevBuf / HostPinned of
csrc/ins_devbuf.h): no other source of libinship names the four runtime calls, and no `*_destroy` function frees memory by hand.  CPU only."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "incompressiblenavierstokes.jl_amd", "csrc")
CALLS = re.compile(r"\b(hipMalloc|hipFree|hipHostMalloc|hipHostFree)\b")
# file name -> why it may name the calls.  Every handle and every temporary of the library has been converted: the seam is the only entry.
ALLOWED = {"ins_devmem.hip": "the seam itself"}
DESTROY = re.compile(r"^[^\n;{}#]*\b(\w+_destroy(?:_f32)?|ins_rk_ext_free)\s*\([^;{}]*\)\s*\{", re.M)


def _code(path):
    src = re.sub(r"/\*.*?\*/", lambda m: re.sub(r"[^\n]", " ", m.group(0)), open(path).read(), flags=re.S)
    return re.sub(r"//[^\n]*", "", src)


def _body(src, start):
    """the text between the brace at `start` and its partner"""
    depth = 0
    for p in range(start, len(src)):
        depth += src[p] == "{"
        depth -= src[p] == "}"
        if depth == 0:
            return src[start:p + 1]
    raise AssertionError("unbalanced braces")


SOURCES = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))


def test_only_the_seam_names_the_allocation_calls():
    assert len(SOURCES) > 50 and all(os.path.exists(os.path.join(CSRC, f)) for f in ALLOWED)
    found = []
    for path in SOURCES:
        name = os.path.basename(path)
        if name in ALLOWED:
            continue
        src = _code(path)
        found += ["%s:%d %s" % (name, src.count("\n", 0, m.start()) + 1, m.group(1)) for m in CALLS.finditer(src)]
    assert not found, "allocate through DevBuf / HostPinned (ins_devbuf.h):\n" + "\n".join(found)


def test_no_destroy_function_frees_by_hand():
    seen = []
    for path in SOURCES:
        src = _code(path)
        for m in DESTROY.finditer(src):
            seen.append(m.group(1))
            body = _body(src, m.end() - 1)
            assert not CALLS.search(body) and "ins_devmem_" not in body, "%s: %s frees memory by hand" % (os.path.basename(path), m.group(1))
    for name in ("ins_grid_destroy", "ins_poisson_destroy", "ins_fdm_destroy", "ins_poisson_destroy_f32", "ins_rk_destroy", "ins_rk_destroy_f32",
                 "ins_rk_ext_free", "adjoint_destroy", "ins_rk_ensemble_destroy", "ins_spectrum_destroy", "ins_slab_fft_destroy"):
        assert name in seen, name
