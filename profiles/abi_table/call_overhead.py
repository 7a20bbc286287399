"""Host cost of one ctypes call before and after the signature table, on two cheap core
functions: tv_hevc_scale_mv (4 ints + 1 host pointer) and tv_bytes_size (1 opaque pointer),
called the way the GPU entry points were called before (no argtypes, pointers wrapped in
c_void_p by hand) and the way they are now (argtypes from thinvids_amd/_abi.py, plain ints).
CPU only.

    python profiles/abi_table/call_overhead.py
"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from thinvids_amd import _native  # noqa: E402

N = 200_000
new = _native.core_lib()
old = C.CDLL(str(_native.LIBDIR / "libtvcore.so"))  # a second handle: nothing declared on it
old.tv_bytes_size.restype = C.c_size_t
out = (C.c_int * 2)()
addr = C.addressof(out)
buf = _native.Bytes()


def per_call(fn):
    best = 1e9
    for _ in range(5):
        t = time.perf_counter()
        for _ in range(N):
            fn()
        best = min(best, (time.perf_counter() - t) / N)
    return best * 1e9


for name, before, after in (
        ("tv_hevc_scale_mv", lambda: old.tv_hevc_scale_mv(7, -3, 2, -2, C.c_void_p(addr)),
         lambda: new.tv_hevc_scale_mv(7, -3, 2, -2, out)),
        ("tv_bytes_size", lambda: old.tv_bytes_size(C.c_void_p(buf.h)), lambda: new.tv_bytes_size(buf.h))):
    print(f"{name}: no argtypes, c_void_p(ptr) {per_call(before):.0f} ns/call; table argtypes {per_call(after):.0f} ns/call")
