"""The library's TIFF reader / writer (dsx_tiff_*, data/tiff.py) on the host: files written by PIL and by a
struct-level writer (tests/tiff_files.py) read back exactly, what the writer emits is read back by PIL, unsupported
layouts are refused by the tag's value, and a corruption sweep ends in an array or an error message, never a crash.
Also the argument refusals of the device entry points that need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import tiff_files as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dsx_tiff_open", "dsx_tiff_info", "dsx_tiff_read", "dsx_tiff_close", "dsx_tiff_write", "dsx_frames_to_f32",
       "dsx_order_stats", "dsx_order_stats_workspace_bytes")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return TF.valid_files(tmp_path_factory.mktemp("tiff"))


def test_every_valid_file_reads_back_exactly(files):
    from diffsplitting_amd.data.tiff import imread
    assert len(files) == 14
    for path, src in files:
        got = imread(path)
        assert got.dtype == src.dtype and got.shape == src.shape, path
        assert got.tobytes() == src.tobytes(), path                 # bitwise: -0.0 and the denormal included
        assert np.array_equal(got, src), path
    u16 = dict((os.path.basename(p), s) for p, s in files)["pil_u16_classic.tif"]
    assert u16.max() == 65535
    f32 = dict((os.path.basename(p), s) for p, s in files)["pil_f32_classic.tif"].reshape(-1)
    assert np.signbit(f32[0]) and f32[0] == 0 and 0 < f32[1] < np.finfo(np.float32).tiny


def test_single_page_keeps_its_leading_one(tmp_path):
    from diffsplitting_amd.data.tiff import imread
    src = TF.source(np.uint16)[:1]
    TF.struct_tiff(tmp_path / "one.tif", list(src))
    assert imread(tmp_path / "one.tif").shape == (1, TF.H, TF.W)
    # an ImageJ description on a file that is too short for its images=N planes: the one page the IFD describes
    TF.struct_tiff(tmp_path / "short.tif", list(src), description="ImageJ=1.53t\nimages=3\n")
    assert np.array_equal(imread(tmp_path / "short.tif"), src)


@pytest.mark.parametrize("dtype", [np.uint16, np.float32, np.uint8])
@pytest.mark.parametrize("big", [None, True])
def test_imwrite_is_read_back_by_pil(tmp_path, dtype, big):
    from PIL import Image
    from diffsplitting_amd.data.tiff import imread, imwrite
    src = TF.source(dtype)
    desc = "ImageJ=1.11a\nimages=3\nchannels=1\nframes=3\nhyperstack=true\nmode=grayscale\n"
    p = tmp_path / "w.tif"
    imwrite(p, src, description=desc, bigtiff=big)
    with open(p, "rb") as f:
        assert f.read(4) == (b"II\x2b\x00" if big else b"II\x2a\x00")
    with Image.open(p) as im:
        assert im.n_frames == 3
        assert im.tag_v2[270] == desc
        for k in range(3):
            im.seek(k)
            page = np.array(im)
            assert page.dtype == src.dtype and page.tobytes() == src[k].tobytes(), k
    assert imread(p).tobytes() == src.tobytes()                     # also as ImageJ's contiguous stack (images=3)
    imwrite(p, src[0])                                              # (H, W), no description
    with Image.open(p) as im:
        assert im.n_frames == 1 and 270 not in im.tag_v2 and np.array_equal(np.array(im), src[0])


def test_unsupported_layouts_are_refused_by_name(tmp_path):
    from diffsplitting_amd._lib import DsxError
    from diffsplitting_amd.data.tiff import imread, imwrite
    u16 = TF.source(np.uint16)
    TF.pil_tiff(tmp_path / "lzw.tif", u16, compression="tiff_lzw")
    TF.struct_tiff(tmp_path / "tiled.tif", list(u16), override={322: (3, [16]), 323: (3, [16])})
    TF.struct_tiff(tmp_path / "planar.tif", list(TF.source(np.uint16, 2)), override={284: (3, [2])})
    TF.struct_tiff(tmp_path / "bits12.tif", list(u16), override={258: (3, [12])})
    TF.struct_tiff(tmp_path / "mixed.tif", [u16[0], u16[1][:30, :20], u16[2]])
    TF.struct_tiff(tmp_path / "signed.tif", list(u16), override={339: (3, [2])})
    for name, pattern in (("lzw", r"Compression = 5 \(LZW\)"), ("tiled", r"tiled.*TileWidth = 16"),
                          ("planar", r"PlanarConfiguration = 2"), ("bits12", r"BitsPerSample = 12"),
                          ("mixed", r"page 1 is 30 x 20 x 1.*page 0 is 37 x 41 x 1"), ("signed", r"SampleFormat = 2")):
        with pytest.raises(DsxError, match=pattern):
            imread(tmp_path / f"{name}.tif")
    with pytest.raises(DsxError, match="cannot be opened"):
        imread(tmp_path / "absent.tif")
    with pytest.raises(DsxError, match="int32"):
        imwrite(tmp_path / "x.tif", np.zeros((1, 4, 4), np.int32))


def test_corruption_sweep_ends_in_an_array_or_a_message(files, tmp_path):
    """Every truncation at k/64 of the length and every one of the first 256 bytes forced to 0x00 / 0xFF: the library
    (unsanitised here; tools/tiff_sanitize.sh runs the same files under ASan + UBSan) returns an array of the shape it
    declared or an error with a message."""
    from diffsplitting_amd import _lib
    lib = _lib.lib
    p = str(tmp_path / "v.tif").encode()
    n_ok = n_refused = 0
    for path, src in files:
        with open(path, "rb") as f:
            data = f.read()
        for name, blob in TF.variants(data):
            with open(p, "wb") as f:
                f.write(blob)
            h = C.c_void_p()
            rc = lib.dsx_tiff_open(p, C.byref(h))
            if rc == 0:
                shape, code = (C.c_int64 * 4)(), C.c_int(-1)
                assert lib.dsx_tiff_info(h, shape, C.byref(code)) == 0
                n, hh, ww, s = (int(v) for v in shape)
                assert n >= 1 and hh >= 1 and ww >= 1 and 1 <= s <= 4 and code.value in (0, 1, 2, 3)
                item = (1, 2, 4, 4)[code.value]
                assert n * hh * ww * s * item <= len(blob)          # never more than the file holds
                out = np.empty(n * hh * ww * s * item, np.uint8)
                rc = lib.dsx_tiff_read(h, 0, n, out.ctypes.data_as(C.c_void_p), out.nbytes)
                lib.dsx_tiff_close(h)
            if rc == 0:
                n_ok += 1
            else:
                assert rc < 0 and len(lib.dsx_last_error()) > 0, (path, name)
                n_refused += 1
    assert n_ok > 0 and n_refused > 14 * 64 // 2                    # most truncations cut into the pixel data


def test_abi_additive():
    from diffsplitting_amd import _lib
    with open(os.path.join(ROOT, "include", "dsx.h")) as f:
        header = f.read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    assert "#define DSX_ABI_VERSION 2" in header and _lib.lib.dsx_abi_version() == 2
    assert _lib.lib.dsx_order_stats_workspace_bytes(10 * 2048 * 2048, 2) <= 1 << 16      # no per-element temporary


def test_device_entry_points_refuse_bad_arguments_without_a_device():
    """Fake non-null device pointers: a call that got past its checks would not come back with these messages."""
    from diffsplitting_amd import _lib
    lib = _lib.lib
    err = lambda: lib.dsx_last_error().decode()
    fake = C.c_void_p(4096)
    out = (C.c_double * 8)()
    ranks = lambda *v: (C.c_int64 * len(v))(*v)
    stats = lambda a, b, count, r, n, o=out, ws=fake: lib.dsx_order_stats(a, b, count, 1.0, 1.0, r, n, o, ws, None)
    assert stats(None, None, 10, ranks(0), 1) < 0 and "null" in err()
    assert stats(fake, None, 10, None, 1) < 0 and "null" in err()
    assert stats(fake, None, 10, ranks(0), 1, o=None) < 0 and "null" in err()
    assert stats(fake, None, 10, ranks(0), 1, ws=None) < 0 and "null" in err()
    assert stats(fake, None, 0, ranks(0), 1) < 0 and "count = 0" in err()
    assert stats(fake, fake, -5, ranks(0), 1) < 0 and "count = -5" in err()
    assert stats(fake, None, 10, ranks(10), 1) < 0 and "rank 10" in err()
    assert stats(fake, None, 10, ranks(3, -1), 2) < 0 and "rank -1" in err()
    assert stats(fake, None, 10, ranks(0), 0) < 0 and "n_ranks = 0" in err()
    assert stats(fake, None, 10 ** 6, (C.c_int64 * 4097)(), 4097, o=(C.c_double * 4097)()) < 0 and "n_ranks = 4097" in err()
    assert lib.dsx_order_stats(fake, fake, 10, float("inf"), 1.0, ranks(0), 1, out, fake, None) < 0 and "finite" in err()
    widen = lambda s, dt, count, d: lib.dsx_frames_to_f32(s, dt, count, 1993.0, d, None)
    assert widen(None, _lib.PIX_U16, 10, fake) < 0 and "null" in err()
    assert widen(fake, _lib.PIX_U16, 10, None) < 0 and "null" in err()
    assert widen(fake, _lib.PIX_U16, 0, fake) < 0 and "count = 0" in err()
    assert widen(fake, _lib.PIX_F32, 10, fake) < 0 and "source type 3" in err()
    assert lib.dsx_frames_to_f32(fake, _lib.PIX_U8, 10, float("nan"), fake, None) < 0 and "NaN" in err()
    # the TIFF entry points
    h = C.c_void_p()
    assert lib.dsx_tiff_open(None, C.byref(h)) < 0 and "null" in err()
    assert lib.dsx_tiff_write(b"/nonexistent-dir/x.tif", fake, 1, 4, 4, _lib.PIX_U8, None, 0) < 0 and "created" in err()
    assert lib.dsx_tiff_write(b"x.tif", fake, 0, 4, 4, _lib.PIX_U8, None, 0) < 0 and "0 pages" in err()
    assert lib.dsx_tiff_write(b"x.tif", fake, 1, 4, 4, _lib.PIX_U32, None, 0) < 0 and "pixel type 2" in err()
    assert lib.dsx_tiff_write(b"x.tif", fake, 3 * 1024, 1024, 1024, _lib.PIX_U16, None, 0) < 0 and "BigTIFF" in err()


def test_split_dataset_reads_tif_on_the_host(files, tmp_path):
    """load_data: channelwise .tif stacks come back clipped at 1993 as the .npy path does; fpath splits unclipped."""
    from diffsplitting_amd.data.split_dataset import DataLocation, load_data
    by_name = dict((os.path.basename(p), (p, s)) for p, s in files)
    p16, s16 = by_name["pil_u16_classic.tif"]
    d = load_data("Hagen", DataLocation(channelwise_fpath=(p16, p16)))
    assert np.array_equal(d[0], np.minimum(s16, 1993)) and d[0].max() == 1993
    np.save(tmp_path / "c.npy", s16)
    n = load_data("Hagen", DataLocation(channelwise_fpath=(str(tmp_path / "c.npy"),) * 2))
    assert n[0].dtype == np.float32 and np.array_equal(n[0], d[0].astype(np.float32))
    p2, s2 = by_name["struct_spp2_u16.tif"]
    f = load_data("Hagen", DataLocation(fpath=p2))
    assert np.array_equal(f[0], s2[..., 0]) and np.array_equal(f[1], s2[..., 1]) and f[0].max() > 1993
