"""ctypes binding of the C-ABI library, read from its public headers (include/rtgs_raster.h, rtgs_debug.h, rtgs_icp.h,
rtgs_slam.h) when this module is imported.

Nothing here restates a declaration: `_cdecl` turns every `typedef struct`, every `rtgs_*(...)` prototype and every
`#define RTGS_NAME <integer>` of the four headers into a ctypes Structure, a (restype, argtypes) pair and an entry of
`CONSTANTS`.  A new entry point or struct member is declared in the header and nowhere else; a declaration outside the
subset the reader understands (the comment at the top of include/rtgs_raster.h) stops the import.

The library is the product: there is NO fallback.  If `librtgs_hip.so` is missing or fails to
load, importing any op raises (build it with `python -c "import __graft_entry__ as g; g.build()"`
or `make -C rtg_slam_amd/csrc`)."""
from __future__ import annotations

import ctypes as C
import os
import threading

import torch

from . import _cdecl

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RTGS_LIB_PATH") or os.path.join(_HERE, "librtgs_hip.so")   # env override: A/B of kernel variants
INCLUDE_DIR = os.path.join(os.path.dirname(_HERE), "include")
HEADERS = ("rtgs_raster.h", "rtgs_debug.h", "rtgs_icp.h", "rtgs_slam.h")


def _read_headers() -> _cdecl.Declarations:
    decl = _cdecl.Declarations()
    for h in HEADERS:
        path = os.path.join(INCLUDE_DIR, h)
        if not os.path.exists(path):
            raise RuntimeError(f"rtg_slam_amd: header not found at {path}. The binding is read from the headers of the "
                               "source tree; there is no second copy of the declarations.")
        try:
            decl.read(open(path).read())
        except _cdecl.CDeclError as e:
            raise RuntimeError(f"rtg_slam_amd: {path}: {e}") from e
    return decl


_decl = _read_headers()
STRUCTS = _decl.structs                      # C name -> ctypes.Structure class
CONSTANTS = _decl.constants                  # "RTGS_NAME" -> int
EXPORTED_SYMBOLS = tuple(_decl.functions)
RasterSettingsC, IcpLevelC, LossCfgC, AttachC, ActivatedC, MapStepArgsC = (STRUCTS[n] for n in (
    "rtgs_raster_settings", "rtgs_icp_level", "rtgs_loss_cfg", "rtgs_attach", "rtgs_activated", "rtgs_map_step_args"))
RESIZE_FN = _decl.callbacks["rtgs_resize_fn"]
FWD_NO_BACKWARD = CONSTANTS["RTGS_FWD_NO_BACKWARD"]

_lock = threading.Lock()
_lib = None


def ptr(t: torch.Tensor):
    """Device pointer of a tensor; None is an error."""
    return C.c_void_p(t.data_ptr())


def ptr0(t):
    """Device pointer of a tensor, NULL for None."""
    return C.c_void_p(None if t is None else t.data_ptr())


def stream(dev):
    """The current HIP stream of `dev` as the `void* stream` every entry point takes."""
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def load():
    """Load (once) and return the ctypes handle; raises RuntimeError when the HIP library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"rtg_slam_amd: native library not found at {LIB_PATH}. There is no CPU fallback; build it "
                "with `make -C rtg_slam_amd/csrc` (hipcc --offload-arch=gfx950).")
        try:
            lib = C.CDLL(LIB_PATH)
        except OSError as e:  # pragma: no cover
            raise RuntimeError(f"rtg_slam_amd: failed to load {LIB_PATH}: {e}") from e
        for name, (res, args) in _decl.functions.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        for what, mirror, size in (("rtgs_map_step_args", MapStepArgsC, lib.rtgs_map_step_args_size()),
                                   ("rtgs_raster_settings", RasterSettingsC, lib.rtgs_raster_settings_size())):
            if C.sizeof(mirror) != size:
                raise RuntimeError(f"rtg_slam_amd: ctypes mirror of {what} is {C.sizeof(mirror)} B, the library says "
                                   f"{size} B - the library was built from other headers than include/*.h of this tree")
        _lib = lib
    return _lib


def check(rc: int, what: str):
    if rc != 0:
        msg = {-1: "invalid argument", -2: "HIP runtime / kernel launch failure", -3: "scratch allocation failed"}.get(rc, "unknown")
        raise RuntimeError(f"{what} failed: {msg} (code {rc})")
