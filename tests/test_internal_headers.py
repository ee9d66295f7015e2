"""CPU-side checks that every function shared between the translation units of libinship is declared once, in a header both sides include (the build's
-Werror=missing-prototypes holds the defining side to it; these hold the calling side and the C hooks):
no csrc/*.hip file carries a prototype of an `ins_` function of its own, every `extern "C"` function is declared in include/ins_hip.h or in
csrc/ins_debug.h, and so is every `ins_dbg_*` / `ins_tune_*` name that _lib.py binds.  The headers are parsed as tests/test_*_abi.py parse ins_hip.h."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "incompressiblenavierstokes.jl_amd")
CSRC = os.path.join(PKG, "csrc")

# a line that starts at column 0 with a type, names an ins_ function and closes its (possibly multi-line) parameter list with `;` instead of a body
PROTOTYPE = re.compile(r"^[A-Za-z_][^;{}()#\n]*?\b(ins_\w+)\s*\([^;{}]*?\)\s*;", re.M)
C_DEFINITION = re.compile(r'^extern\s+"C"\s+[^;{}()#\n]*?\b(\w+)\s*\([^;{}]*?\)\s*\{', re.M)


def _code(path):
    """The file without comments; line breaks are kept, so a match's line number is the file's."""
    src = re.sub(r"/\*.*?\*/", lambda m: re.sub(r"[^\n]", " ", m.group(0)), open(path).read(), flags=re.S)
    return re.sub(r"//[^\n]*", "", src)


def _declared(name, *headers):
    return any(re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, _code(h)) for h in headers)


PUBLIC = os.path.join(ROOT, "include", "ins_hip.h")
DEBUG = os.path.join(CSRC, "ins_debug.h")
UNITS = sorted(glob.glob(os.path.join(CSRC, "*.hip")))


def test_prototype_pattern_sees_what_it_must():
    copies = ("int ins_k_a(const ins_grid* G, hipStream_t s);\n"
              "int ins_k_b(const ins_grid* G, double* u,\n                  int part = 0);\n"
              'extern "C" long long ins_dbg_c(void);\n'
              "const ins_grid* ins_k32_d(const ins_poisson32* ps);\n")
    assert [m.group(1) for m in PROTOTYPE.finditer(copies)] == ["ins_k_a", "ins_k_b", "ins_dbg_c", "ins_k32_d"]
    uses = ("int ins_k_a(const ins_grid* G, hipStream_t s) {\n  return ins_k_b(G, nullptr);\n}\n"
            "bool ins_e(int n) { return n > 0; }\n"
            "#define CALL(x) ins_k_a(x, s);\n")
    assert not PROTOTYPE.search(uses)


def test_no_unit_declares_an_ins_function_itself():
    assert len(UNITS) >= 37
    found = []
    for path in UNITS:
        src = _code(path)
        found += ["%s:%d %s" % (os.path.basename(path), src.count("\n", 0, m.start()) + 1, m.group(1)) for m in PROTOTYPE.finditer(src)]
    assert not found, "prototypes that belong in ins_internal.h, ins_f32_internal.h or ins_debug.h:\n" + "\n".join(found)


def test_every_c_function_is_declared_in_a_header():
    defined = []
    for path in UNITS:
        src = _code(path)
        assert not re.search(r'extern\s+"C"\s*\{', src), os.path.basename(path)  # definitions carry the linkage one by one: the pattern sees them all
        assert len(C_DEFINITION.findall(src)) == len(re.findall(r'^extern\s+"C"', src, re.M)), os.path.basename(path)
        defined += C_DEFINITION.findall(src)
    assert len(defined) > 200 and len(set(defined)) == len(defined)
    missing = [n for n in defined if not _declared(n, PUBLIC, DEBUG)]
    assert not missing, missing
    # the hook header declares nothing the public header has, and nothing that is not defined
    hooks = re.findall(r"\b(ins_\w+)\s*\([^)]*\)\s*;", _code(DEBUG))
    assert hooks and all(re.match(r"ins_(dbg|tune)_", n) for n in hooks)
    assert not [n for n in hooks if n not in defined or _declared(n, PUBLIC)]


def test_every_bound_hook_is_declared():
    bound = set(re.findall(r"""["'](ins_(?:dbg|tune)_\w+)["']""", open(os.path.join(PKG, "_lib.py")).read()))
    assert bound
    assert not [n for n in sorted(bound) if not _declared(n, PUBLIC, DEBUG)]
