"""The ctypes signature table (thinvids_amd/_abi.py) against the C sources it describes: a small
prototype parser reads every `extern "C"` `tv_*` definition under csrc/core and csrc/gpu, and
the table must name exactly those functions with exactly those types.  The parser is checked
against the dynamic symbols of the built libraries, so it cannot skip a definition silently."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from thinvids_amd import _abi, _native

ROOT = Path(__file__).resolve().parent.parent
GENERATED = {"tv_core_build_hash", "tv_gpu_build_hash"}  # emitted by _build._stamp_obj

# C scalar -> ctypes type: exact for a scalar parameter, element size and kind for a pointee
TYPES = {
    "int": C.c_int, "long": C.c_long, "long long": C.c_longlong, "size_t": C.c_size_t, "uint32_t": C.c_uint32,
    "int32_t": C.c_int32, "int64_t": C.c_int64, "unsigned long long": C.c_ulonglong, "float": C.c_float,
    "uint8_t": C.c_uint8, "int8_t": C.c_int8, "uint16_t": C.c_uint16, "int16_t": C.c_int16, "uint64_t": C.c_uint64,
    "double": C.c_double,
}
TYPE_WORDS = {"void", "char", "int", "long", "unsigned", "float", "double"}
PROTO = re.compile(r'^(?:extern\s+"C"\s+)?((?:const\s+)?[A-Za-z_][\w ]*?[\s*]+)(tv_\w+)\s*\(([^()]*)\)\s*\{', re.M)


def _ctype(decl: str, named: bool) -> str:
    """'const uint8_t* const* segs' -> 'uint8_t**'; 'unsigned long long pmask' -> 'unsigned long long'."""
    assert not re.search(r"[^\w\s*]", decl), decl  # no arrays, references, defaults or callbacks
    toks = [t for t in re.findall(r"\w+|\*", decl) if t != "const"]
    if named and toks[-1] != "*" and toks[-1] not in TYPE_WORDS and not toks[-1].endswith("_t"):
        toks.pop()  # the parameter's name
    return " ".join(t for t in toks if t != "*") + "*" * toks.count("*")


def parse(which: str) -> dict:
    """{name: (return type, [parameter types])} of the exported tv_* definitions, comments stripped."""
    out = {}
    for path in sorted((ROOT / "csrc" / which).glob("*.cpp" if which == "core" else "*.hip")):
        text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", " ", path.read_text(), flags=re.S))
        for m in PROTO.finditer(text):
            ret, name, params = m.group(1), m.group(2), m.group(3).strip()
            if re.match(r"\s*(static|inline)\b", ret):
                continue
            assert name not in out, f"{name} defined twice"
            out[name] = (_ctype(ret, False), [] if params in ("", "void") else [_ctype(p, True) for p in params.split(",")])
    return out


def _kind(t):
    return C.sizeof(t), "f" if t in (C.c_float, C.c_double) else "i" if t(-1).value < 0 else "u"


def _type_ok(ctype: str, t) -> bool:
    if not ctype.endswith("*"):
        return t is (None if ctype == "void" else TYPES[ctype])
    pointee = ctype[:-1]
    if t is C.c_void_p or (t is C.c_char_p and pointee == "char"):
        return True
    if not (isinstance(t, type) and issubclass(t, C._Pointer)):
        return False
    el = t._type_
    if pointee.endswith("*"):
        return el is C.c_void_p or issubclass(el, C._Pointer)
    if pointee in TYPES:
        return _kind(el) == _kind(TYPES[pointee])
    return issubclass(el, C.Structure) and el.__name__ == pointee  # the Python mirror carries the C name


@pytest.mark.parametrize("lib", ["libtvcore", "libtvgpu"])  # (an id "gpu" would read as the gpu marker)
def test_table_equals_source(lib):
    which = lib[5:]
    table = _abi.CORE if which == "core" else _abi.GPU
    src = parse(which)
    assert set(table) - GENERATED == set(src)
    assert set(table) & GENERATED == {f"tv_{which}_build_hash"}
    bad = []
    for name, (ret, args) in sorted(src.items()):
        res, argtypes = table[name]
        if len(args) != len(argtypes):
            bad.append(f"{name}: {len(args)} parameters in C, {len(argtypes)} in the table")
            continue
        bad += [f"{name}: {'returns' if k < 0 else f'parameter {k} is'} {a}, table says {t}"
                for k, (a, t) in enumerate(zip([ret] + args, [res] + argtypes), -1) if not _type_ok(a, t)]
    assert not bad, "\n".join(bad)


def test_parser_handles_the_forms_in_use():
    core, gpu = parse("core"), parse("gpu")
    assert core["tv_hevc_spec_table"] == ("int", ["char*", "int*", "int"])  # single-line extern "C" int tv_...(
    assert gpu["tv_ssim_plane"][1][:3] == ["uint8_t*", "uint8_t*", "int"]  # ... continued over two lines
    assert core["tv_mux_mp4_file"][1][0] == "uint8_t**"  # const T* const*
    assert "unsigned long long" in gpu["tv_gpu_cdef_search"][1]
    assert core["tv_mux_file"][1].count("SideTrack*") == 1
    assert len(gpu["tv_av1e_inter"][1]) == 23  # multi-line parameter list


def test_parser_sees_every_exported_symbol():
    """Parsed definitions == the defined dynamic tv_* symbols of libtvcore.so, and of
    libtvgpu.so when it has been built (nm only reads the file: no GPU needed)."""
    nm = shutil.which("nm")
    if nm is None:
        pytest.skip("no nm on this machine")
    _native.core_lib()  # builds libtvcore.so if need be
    for which, table in (("core", _abi.CORE), ("gpu", _abi.GPU)):
        path = _native.LIBDIR / f"libtv{which}.so"
        if which == "gpu" and not path.exists():
            continue
        out = subprocess.run([nm, "-D", "--defined-only", str(path)], check=True, capture_output=True, text=True).stdout
        syms = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("tv_")}
        assert syms - GENERATED == set(parse(which)), which
        assert syms == set(table), which


DECL = re.compile(r"[\w)\]]\s*\.\s*(?:argtypes|restype)\b[^=\n]*=(?!=)")
# _native._sig applies the table; libavif and roctx are third-party libraries with bindings of their own
MAY_DECLARE = {"thinvids_amd/_native.py", "thinvids_amd/models/avif.py", "thinvids_amd/utils/trace.py"}


def test_no_stray_declarations():
    """Signatures of tv_* functions live in _abi.py only: nothing else assigns an `.argtypes`
    or a `.restype`, whether on `lib.tv_x`, on an alias of it or on `getattr(lib, name)`."""
    bad = []
    for path in [ROOT / "bench.py", *(p for d in ("thinvids_amd", "tests", "tools") for p in (ROOT / d).rglob("*.py"))]:
        rel = path.relative_to(ROOT).as_posix()
        if rel in MAY_DECLARE or path == Path(__file__).resolve():
            continue
        bad += [f"{rel}: {m.group(0)}" for m in DECL.finditer(path.read_text())]
    assert not bad, "\n".join(bad)
    assert len(DECL.findall((ROOT / "thinvids_amd" / "_native.py").read_text())) == 2  # the two lines of _sig


def test_each_name_declared_once():
    text = (ROOT / "thinvids_amd" / "_abi.py").read_text()
    names = re.findall(r'^\s*"(tv_\w+)"\s*:', text, re.M)
    assert len(names) == len(set(names)), sorted(n for n in set(names) if names.count(n) > 1)
    assert set(names) == set(_abi.CORE) | set(_abi.GPU)
    assert not set(_abi.CORE) & set(_abi.GPU)


def test_ctypes_refuses_bad_calls():
    lib = _native.core_lib()
    with pytest.raises((TypeError, C.ArgumentError)):
        lib.tv_satd8x8((C.c_int * 64)())  # one argument too few
    with pytest.raises((TypeError, C.ArgumentError)):
        lib.tv_satd8x8((C.c_int * 64)(), 8.0)  # a float for an int


@pytest.mark.gpu
def test_gpu_library_resolves_the_table():
    lib = _native.gpu_lib()  # applies GPU: a missing symbol raises here
    assert lib.tv_gpu_device_count() >= 1
