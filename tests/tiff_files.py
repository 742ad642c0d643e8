"""TIFF files for the reader's tests, made by two writers that share no code with the library: PIL, and a struct-level
writer for what PIL cannot produce (big-endian, several strips with a ragged last one, SamplesPerPixel = 2, ImageJ's
contiguous stack, and the layouts the reader must refuse).  ``python tests/tiff_files.py DIR`` writes every valid file
and its corruption sweep into DIR: the input of the sanitised stand-alone reader (tools/tiff_sanitize.sh)."""
import os
import struct
import sys

import numpy as np

PAGES, H, W = 3, 37, 41
_FMT = {1: "B", 3: "H", 4: "I", 16: "Q"}


def source(dtype, samples=1, seed=5):
    """The (3, 37, 41[, S]) source array of a dtype, with the values that an off-by-one in a cast would lose."""
    rng = np.random.default_rng(seed)
    shape = (PAGES, H, W) if samples == 1 else (PAGES, H, W, samples)
    if np.dtype(dtype) == np.float32:
        a = rng.normal(0.0, 1000.0, size=shape).astype(np.float32)
        a.reshape(-1)[:4] = np.array([-0.0, 1e-42, np.finfo(np.float32).max, -np.finfo(np.float32).max], np.float32)
        return a
    top = np.iinfo(dtype).max
    a = rng.integers(0, int(top) + 1, size=shape, dtype=np.uint64).astype(dtype)
    a.reshape(-1)[:2] = (top, 0)
    return a


def pil_tiff(path, arr, big=False, **kw):
    from PIL import Image
    ims = [Image.fromarray(p) for p in arr]
    ims[0].save(path, format="TIFF", save_all=True, append_images=ims[1:], big_tiff=big, **kw)


def struct_tiff(path, pages, order="<", rows_per_strip=None, big=False, imagej=False, override=None, description=None):
    """``pages``: arrays (H, W) or (H, W, S), possibly of differing shape.  ``override``: {tag: (type, [values])}
    replaces or adds IFD entries.  ``imagej``: every page's data back to back, ONE IFD, description ImageJ=...images=N."""
    E = order
    out = bytearray((b"II" if E == "<" else b"MM") + (struct.pack(E + "HHHQ", 43, 8, 0, 0) if big else struct.pack(E + "HI", 42, 0)))
    ptr_at, ptr_fmt = (8, "Q") if big else (4, "I")              # where the offset of the next IFD goes
    inline, cnt_fmt, n_fmt = (8, "Q", "Q") if big else (4, "I", "H")
    metas = []
    for p in pages:
        a = np.ascontiguousarray(p)
        raw = a.astype(a.dtype.newbyteorder(E)).tobytes()
        h, w = a.shape[:2]
        s = a.shape[2] if a.ndim == 3 else 1
        rps = rows_per_strip or h
        rowb = len(raw) // h
        offs, cnts = [], []
        for r0 in range(0, h, rps):
            chunk = raw[r0 * rowb:min(h, r0 + rps) * rowb]
            offs.append(len(out)); cnts.append(len(chunk)); out += chunk
        metas.append({256: (4, [w]), 257: (4, [h]), 258: (3, [a.dtype.itemsize * 8] * s), 259: (3, [1]), 262: (3, [1]),
                      273: (16 if big else 4, offs), 277: (3, [s]), 278: (4, [rps]), 279: (16 if big else 4, cnts),
                      284: (3, [1]), 339: (3, [3 if a.dtype.kind == "f" else 1] * s)})
    if imagej:
        metas = metas[:1]
        description = f"ImageJ=1.53t\nimages={len(pages)}\nslices={len(pages)}\n"
    if description is not None:
        metas[0][270] = (2, description.encode() + b"\0")
    for m in metas:
        m.update(override or {})
        fields = []
        for tag in sorted(m):
            typ, vals = m[tag]
            data = bytes(vals) if typ == 2 else struct.pack(E + _FMT[typ] * len(vals), *vals)
            if len(data) > inline:
                out += b"\0" * (len(out) % 2)
                at = len(out)
                out += data
                data = struct.pack(E + ptr_fmt, at)
            fields.append(struct.pack(E + "HH" + cnt_fmt, tag, typ, len(vals)) + data.ljust(inline, b"\0"))
        out += b"\0" * (len(out) % 2)
        out[ptr_at:ptr_at + inline] = struct.pack(E + ptr_fmt, len(out))
        out += struct.pack(E + n_fmt, len(fields)) + b"".join(fields)
        ptr_at = len(out)
        out += struct.pack(E + ptr_fmt, 0)
    with open(path, "wb") as f:
        f.write(out)


def valid_files(directory):
    """Writes the valid files -> [(path, source array)]."""
    d = str(directory)
    made = []
    for name, dt in (("u16", np.uint16), ("u8", np.uint8), ("f32", np.float32)):
        for big in (False, True):
            p = os.path.join(d, f"pil_{name}_{'big' if big else 'classic'}.tif")
            pil_tiff(p, source(dt), big=big)
            made.append((p, source(dt)))
    cases = {"be_u16": dict(dt=np.uint16, order=">"), "be_f32_big": dict(dt=np.float32, order=">", big=True),
             "strips_u16": dict(dt=np.uint16, rows_per_strip=5), "strips_be_f32": dict(dt=np.float32, order=">", rows_per_strip=8),
             "spp2_u16": dict(dt=np.uint16, samples=2, rows_per_strip=16), "imagej_u16": dict(dt=np.uint16, imagej=True),
             "imagej_big_f32": dict(dt=np.float32, imagej=True, big=True, rows_per_strip=10), "u32": dict(dt=np.uint32)}
    for name, c in cases.items():
        c = dict(c)
        src = source(c.pop("dt"), c.pop("samples", 1))
        p = os.path.join(d, f"struct_{name}.tif")
        struct_tiff(p, list(src), **c)
        made.append((p, src))
    return made


def variants(data):
    """The corruption sweep of one file's bytes: truncated at every 1/64 of its length, and each of its first 256
    bytes set to 0x00 and to 0xFF, one byte at a time -> (name, bytes)."""
    for k in range(64):
        yield f"trunc{k:02d}", data[:len(data) * k // 64]
    for i in range(min(256, len(data))):
        for v in (0x00, 0xFF):
            if data[i] != v:
                b = bytearray(data)
                b[i] = v
                yield f"byte{i:03d}_{v:02x}", bytes(b)


if __name__ == "__main__":
    dest = sys.argv[1]
    os.makedirs(dest, exist_ok=True)
    count = 0
    for path, _ in valid_files(dest):
        count += 1
        with open(path, "rb") as f:
            data = f.read()
        stem = os.path.splitext(path)[0]
        for name, blob in variants(data):
            with open(f"{stem}.{name}.tif", "wb") as f:
                f.write(blob)
            count += 1
    print(count)
