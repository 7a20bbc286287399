"""ctypes bindings to the in-tree native libraries (``_lib/libtvcore.so``, ``_lib/libtvgpu.so``).

The libraries are built by :mod:`thinvids_amd._build` (``__graft_entry__.build()``).  On a
GPU box the GPU library is REQUIRED by the GPU engine: :func:`gpu_lib` raises instead of
falling back to anything else, so a missing build fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from pathlib import Path

import numpy as np

from . import _abi

LIBDIR = Path(__file__).resolve().parent / "_lib"
_lock = threading.Lock()
_core = None
_gpu = None
_ptr_types: dict = {}  # numpy dtype -> ctypes pointer type, for ptr()



def _which(name: str) -> str:
    return "core" if name == "libtvcore.so" else "gpu"


def _embedded_ok(path: Path, digest: str) -> bool:
    """The library's exported build hash (a string literal in .rodata) equals `digest`."""
    try:
        return digest.encode() in path.read_bytes()
    except OSError:
        return False


def _ensure_built(name: str) -> Path:
    """Return the library path, guaranteeing it was built from the CURRENT sources: the
    content hash embedded at link time must match the hash of csrc/ now.  A missing or
    stale library is rebuilt (TV_NO_AUTOBUILD=1: refused loudly instead)."""
    from . import _build

    path = LIBDIR / name
    have_src = (_build.CSRC / "core").is_dir()
    want = _build.expected_hash(_which(name)) if have_src else None
    if want is not None and not _embedded_ok(path, want):
        if os.environ.get("TV_NO_AUTOBUILD") == "1":
            state = "stale (built from other sources)" if path.exists() else "missing"
            raise RuntimeError(f"native library {path} is {state}; run `python -m thinvids_amd._build`")
        if name == "libtvcore.so":
            _build.build_core()
        else:
            _build.build_gpu()
        if not _embedded_ok(path, want):
            raise RuntimeError(f"native library {path} does not match the sources after a rebuild")
    if not path.exists():
        raise RuntimeError(f"native library {path} is missing; run `python -m thinvids_amd._build`")
    return path


def build_hash(lib, which: str) -> str:
    return getattr(lib, f"tv_{which}_build_hash")().decode()


def _sig(lib, name, res, args):
    f = getattr(lib, name)
    f.restype = res
    f.argtypes = args
    return f


def _load(name: str, table: dict):
    """dlopen `name` and declare every function of `table` (a missing symbol fails the load)."""
    lib = C.CDLL(str(_ensure_built(name)), mode=C.RTLD_GLOBAL)
    for fn, (res, args) in table.items():
        _sig(lib, fn, res, args)
    return lib


def core_lib():
    global _core
    if _core is None:
        with _lock:
            if _core is None:
                lib = _load("libtvcore.so", _abi.CORE)
                if lib.tv_side_track_size() != C.sizeof(_abi.SideTrack):
                    raise RuntimeError("SideTrack layout mismatch between Python and libtvcore")
                _core = lib
    return _core


def check(rc: int) -> None:
    ok(rc, core_lib(), "tv_last_error")


def ptr(a: np.ndarray):
    """Typed pointer to a host array, by its dtype: the table's argtype then refuses an array of another type."""
    assert a.flags["C_CONTIGUOUS"], "array must be C-contiguous"
    t = _ptr_types.get(a.dtype) or _ptr_types.setdefault(a.dtype, C.POINTER(np.ctypeslib.as_ctypes_type(a.dtype)))
    return a.ctypes.data_as(t)


class Bytes:
    """Owning handle around a native byte vector."""

    def __init__(self):
        self.lib = core_lib()
        self.h = self.lib.tv_bytes_new()

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.tv_bytes_free(self.h)
            self.h = None

    def tobytes(self) -> bytes:
        n = self.lib.tv_bytes_size(self.h)
        if n == 0:
            return b""
        return C.string_at(self.lib.tv_bytes_data(self.h), n)

    def clear(self) -> None:
        self.lib.tv_bytes_clear(self.h)


def gpu_lib():
    """Load libtvgpu.so (HIP kernels + GPU engine).  Raises if it cannot be loaded."""
    global _gpu
    if _gpu is None:
        core_lib()
        with _lock:
            if _gpu is None:
                _gpu = _load("libtvgpu.so", _abi.GPU)
    return _gpu


def dptr(t) -> int:
    """Device address of a torch tensor, for a `c_void_p` parameter."""
    return t.data_ptr()


def stream(device) -> int:
    """Handle of torch's current stream on `device`, for a `c_void_p` stream parameter."""
    import torch

    return torch.cuda.current_stream(device).cuda_stream


def ok(rc: int, lib, last_error: str, exc=RuntimeError) -> None:
    """Raise `exc` with the message of `lib.<last_error>()` (a `tv_*_last_error`) if rc != 0."""
    if rc != 0:
        raise exc(getattr(lib, last_error)().decode())
