"""Loader for the CPU-native codec hot loops (``csrc/codec_native.c``).

Plain cc + ctypes — deliberately independent of torch and the HIP
extension so the data layer stays importable on any machine.  If the
shared library is missing it is built on demand (sub-second); if no
compiler is available the pure-NumPy paths take over silently.

``RAFT_AMD_PURE_CODEC=1`` forces the pure paths (used by the parity
tests, which check native == pure bit-exactly).
"""
from __future__ import annotations

import ctypes
import os
import subprocess
import tempfile
from typing import Optional

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
_SO = os.path.join(_CSRC, "_codec_native.so")
_lib = None   # None = not tried, False = unavailable


def _declare(lib: ctypes.CDLL) -> ctypes.CDLL:
    u8p = ctypes.POINTER(ctypes.c_uint8)
    i32p = ctypes.POINTER(ctypes.c_int32)
    i64p = ctypes.POINTER(ctypes.c_int64)
    u64p = ctypes.POINTER(ctypes.c_uint64)
    lib.png_unfilter.restype = ctypes.c_int
    lib.png_unfilter.argtypes = [u8p, u8p, ctypes.c_int64, ctypes.c_int64,
                                 ctypes.c_int64, u8p]
    lib.jpeg_baseline_scan.restype = ctypes.c_int
    lib.jpeg_baseline_scan.argtypes = [
        u8p, i64p, ctypes.c_int64,                    # segdata, starts, n
        ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,   # ri, mcus_x/y
        ctypes.c_int64, i32p, i32p, u64p, i32p,       # ncomp, hv, cols,
        u8p, u8p, ctypes.c_int64]                     # addrs, tabs...
    lib.jpeg_prog_dc_scan.restype = ctypes.c_int
    lib.jpeg_prog_dc_scan.argtypes = [
        u8p, i64p, ctypes.c_int64,                    # segdata, starts, n
        ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int,
        ctypes.c_int64, i32p, i32p, i32p, u64p, i32p,  # ncomp, hv, cols,
        u8p, u8p, ctypes.c_int64,                     # nbw, addrs, dc_idx
        ctypes.c_int, ctypes.c_int]                   # al, first
    lib.jpeg_encode_scan.restype = ctypes.c_int64
    lib.jpeg_encode_scan.argtypes = [
        u64p, ctypes.c_int64, ctypes.c_int64,         # zz addrs, mcus x/y
        ctypes.c_int64, i32p, i32p,                   # ncomp, hv, cols
        i32p, u8p, u8p, ctypes.c_int64,               # tab idx/bits/vals
        u8p, ctypes.c_int64]                          # out, cap
    lib.jpeg_prog_ac_scan.restype = ctypes.c_int
    lib.jpeg_prog_ac_scan.argtypes = [
        u8p, i64p, ctypes.c_int64,                    # segdata, starts, n
        ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
        ctypes.c_uint64, u8p, u8p,                    # coef addr, ac tab
        ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    return lib


def build_native(verbose: bool = False) -> Optional[str]:
    """Compile codec_native.c -> _codec_native.so in-tree (atomic)."""
    src = os.path.join(_CSRC, "codec_native.c")
    if not os.path.exists(src):
        return None
    for cc in ("cc", "gcc", "clang"):
        tmp = None          # stays None when the tree is not writable
        try:
            with tempfile.NamedTemporaryFile(
                    dir=_CSRC, suffix=".so", delete=False) as tf:
                tmp = tf.name
            r = subprocess.run(
                [cc, "-O3", "-shared", "-fPIC", "-std=c99", src, "-o", tmp],
                capture_output=True, timeout=120)
            if r.returncode == 0:
                os.replace(tmp, _SO)          # atomic under concurrency
                if verbose:
                    print(f"built {_SO} with {cc}")
                return _SO
            os.unlink(tmp)
        except (OSError, subprocess.TimeoutExpired):
            try:
                if tmp is not None:
                    os.unlink(tmp)
            except OSError:
                pass
            continue
    return None


def lib() -> Optional[ctypes.CDLL]:
    """The loaded native library, or None (pure-NumPy fallback)."""
    global _lib
    if os.environ.get("RAFT_AMD_PURE_CODEC") == "1":
        return None
    if _lib is None:
        try:
            _lib = _declare(ctypes.CDLL(_SO))
        except OSError:
            _lib = False
            if build_native() is not None:
                try:
                    _lib = _declare(ctypes.CDLL(_SO))
                except OSError:
                    _lib = False
    return _lib or None
