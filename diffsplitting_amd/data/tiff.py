"""``.tif`` frame stacks through the library's own reader / writer (``dsx_tiff_*``, include/dsx.h): what the reference
gets from ``imread(fpath, plugin='tifffile')`` (data/split_dataset.py:76-91) for the files its Hagen configs name --
uncompressed classic TIFF / BigTIFF stacks, ImageJ's contiguous stacks included -- and the writer of the stitched
prediction.  Host code: works without a GPU.  Compressed, tiled and planar files are refused with the tag's value.
"""
import ctypes as C

import numpy as np

from .. import _lib
from .._lib import DsxError, check, lib

_DTYPES = {_lib.PIX_U8: np.uint8, _lib.PIX_U16: np.uint16, _lib.PIX_U32: np.uint32, _lib.PIX_F32: np.float32}
_CODES = {np.dtype(np.uint8): _lib.PIX_U8, np.dtype(np.uint16): _lib.PIX_U16, np.dtype(np.float32): _lib.PIX_F32}


def imread(path):
    """-> (N, H, W), or (N, H, W, S) for S > 1 samples per pixel, in the file's own dtype (uint8 / uint16 / uint32 /
    float32).  A single page keeps its leading 1."""
    h = C.c_void_p()
    check(lib.dsx_tiff_open(str(path).encode(), C.byref(h)))
    try:
        shape, code = (C.c_int64 * 4)(), C.c_int()
        check(lib.dsx_tiff_info(h, shape, C.byref(code)))
        n, H, W, S = (int(v) for v in shape)
        out = np.empty((n, H, W) if S == 1 else (n, H, W, S), dtype=_DTYPES[code.value])
        check(lib.dsx_tiff_read(h, 0, n, out, out.nbytes))
        return out
    finally:
        lib.dsx_tiff_close(h)


def imwrite(path, array, description=None, bigtiff=None):
    """(N, H, W) or (H, W) uint8 / uint16 / float32 -> uncompressed little-endian pages, one strip each.
    ``description`` becomes page 0's ImageDescription; ``bigtiff`` None switches to BigTIFF past 4 GiB."""
    a = np.asarray(array)
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3 or a.dtype not in _CODES:
        raise DsxError(f"imwrite: (N, H, W) uint8 / uint16 / float32 expected, got {a.shape} {a.dtype}")
    a = np.ascontiguousarray(a)
    desc = None if description is None else str(description).encode()
    check(lib.dsx_tiff_write(str(path).encode(), a, a.shape[0], a.shape[1], a.shape[2],
                             _CODES[a.dtype], desc, -1 if bigtiff is None else int(bool(bigtiff))))
