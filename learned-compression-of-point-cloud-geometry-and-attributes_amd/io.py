"""PLY in / out for voxelised colour point clouds (host-side IO; numpy only).

The reference reads frames with ``open3d.io.read_point_cloud`` (data/utils/RawLoader.py:46,
metrics/metric.py:50) and writes them with ``o3d.t.io.write_point_cloud`` (model/model.py:326-330);
open3d is not available here.  Supported: ``format ascii 1.0`` and ``format binary_little_endian 1.0``
(8iVFB / MVUB / G-PCC output), one ``vertex`` element whose properties include x, y, z and,
optionally, red / green / blue (uchar) — any further properties (normals, alpha, ...) are skipped.
A cloud is a float32 ``[N, 6]`` array: voxel coordinates and rgb in [0, 1] — the layout
``ColorModel.compress`` takes (model/model.py:95-123).

``write_png`` writes the rendered views of the view-dependent evaluation (evaluate_view_dep.py:346,
``capture_screen_image``) with the standard library alone: no imaging package is assumed.  ``read_png`` reads 8-bit
non-interlaced PNGs the same way: the painted masks and saliency maps of the screen-space quality maps.
"""
import struct
import zlib

import numpy as np

_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
          "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
          "double": "f8", "float64": "f8"}


def _parse_header(f):
    if f.readline().strip() != b"ply":
        raise ValueError("not a PLY file")
    fmt, n_vertex, props, in_vertex, other_elements = None, None, [], False, False
    while True:
        line = f.readline()
        if not line:
            raise ValueError("PLY: header is not terminated")
        tok = line.decode("ascii", "replace").split()
        if not tok or tok[0] == "comment" or tok[0] == "obj_info":
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            in_vertex = tok[1] == "vertex"
            if in_vertex:
                if other_elements:
                    raise ValueError("PLY: the vertex element must come first")
                n_vertex = int(tok[2])
            else:
                other_elements = True
        elif tok[0] == "property" and in_vertex:
            if tok[1] == "list":
                raise ValueError("PLY: list properties on vertices are not supported")
            if tok[1] not in _TYPES:
                raise ValueError("PLY: unknown property type %r" % tok[1])
            props.append((tok[2], _TYPES[tok[1]]))
        elif tok[0] == "end_header":
            break
    if fmt not in ("ascii", "binary_little_endian") or n_vertex is None:
        raise ValueError("PLY: unsupported format %r" % fmt)
    names = [p[0] for p in props]
    if not all(a in names for a in "xyz"):
        raise ValueError("PLY: vertices need x, y, z")
    return fmt, n_vertex, props


def read_ply(path):
    """-> float32 [N, 6] (x, y, z, r, g, b with colours scaled to [0, 1]; zeros when the file has none)."""
    with open(path, "rb") as f:
        fmt, n, props = _parse_header(f)
        names = [p[0] for p in props]
        if fmt == "ascii":
            table = np.loadtxt(f, dtype=np.float64, max_rows=n, ndmin=2) if n else np.zeros((0, len(props)))
            if table.shape != (n, len(props)):
                raise ValueError("PLY: expected %d vertices with %d properties" % (n, len(props)))
            col = lambda name: table[:, names.index(name)]
        else:
            dt = np.dtype([(nm, "<" + t) for nm, t in props])
            raw = np.frombuffer(f.read(n * dt.itemsize), dtype=dt)
            if raw.shape[0] != n:
                raise ValueError("PLY: truncated vertex data")
            col = lambda name: raw[name].astype(np.float64)
        out = np.zeros((n, 6), dtype=np.float32)
        for i, a in enumerate("xyz"):
            out[:, i] = col(a)
        if all(c in names for c in ("red", "green", "blue")):
            for i, c in enumerate(("red", "green", "blue")):
                v = col(c)
                is_byte = dict(props)[c] in ("u1", "i1")
                out[:, 3 + i] = v / 255.0 if is_byte else v
    return out


def write_ply(path, cloud, binary=True):
    """cloud: [N, 3] or [N, 6] (rgb in [0, 1]); coordinates are written as float, colours as uchar."""
    c = np.asarray(cloud, dtype=np.float64)
    has_rgb = c.shape[1] >= 6
    n = c.shape[0]
    head = ["ply", "format %s 1.0" % ("binary_little_endian" if binary else "ascii"), "element vertex %d" % n,
            "property float x", "property float y", "property float z"]
    if has_rgb:
        head += ["property uchar red", "property uchar green", "property uchar blue"]
    head.append("end_header")
    rgb = np.clip(np.round(c[:, 3:6] * 255.0), 0, 255).astype(np.uint8) if has_rgb else None
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        if binary:
            fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")] + ([("red", "u1"), ("green", "u1"), ("blue", "u1")] if has_rgb else [])
            rec = np.zeros(n, dtype=np.dtype(fields))
            rec["x"], rec["y"], rec["z"] = c[:, 0], c[:, 1], c[:, 2]
            if has_rgb:
                rec["red"], rec["green"], rec["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
            f.write(rec.tobytes())
        else:
            for i in range(n):
                row = "%g %g %g" % (c[i, 0], c[i, 1], c[i, 2])
                if has_rgb:
                    row += " %d %d %d" % (rgb[i, 0], rgb[i, 1], rgb[i, 2])
                f.write((row + "\n").encode("ascii"))


def write_png(path, img):
    """img: uint8 [H, W, 3] (array or tensor) -> an 8-bit RGB PNG, non-interlaced, every scanline with filter type 0."""
    if hasattr(img, "detach"):
        img = img.detach().cpu().numpy()
    a = np.ascontiguousarray(img)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("write_png: an image is a uint8 [H, W, 3] array")
    h, w = a.shape[:2]
    rows = np.zeros((h, 1 + 3 * w), dtype=np.uint8)          # a filter byte (0 = none) in front of every scanline
    rows[:, 1:] = a.reshape(h, 3 * w)

    def chunk(tag, body):
        return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + chunk(b"IEND", b""))


_PNG_CHANNELS = {0: 1, 2: 3, 4: 2, 6: 4}          # colour type -> samples per pixel: grey, RGB, grey + alpha, RGBA


def read_png(path):
    """An 8-bit non-interlaced PNG (a path or its bytes) -> uint8 [H, W] for grey, [H, W, 2] for grey + alpha, [H, W, 3] for RGB,
    [H, W, 4] for RGBA: what a painted mask or a saliency map comes as (tools/view_dep.py --screen-mask), and what ``write_png``
    writes.  All five scanline filters; every chunk's CRC is checked; ancillary chunks are skipped.  ValueError for anything
    else: a palette, another bit depth, interlacing, a damaged file."""
    if isinstance(path, (bytes, bytearray, memoryview)):
        raw = bytes(path)
    else:
        with open(path, "rb") as f:
            raw = f.read()
    if raw[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError("read_png: not a PNG (bad signature)")
    pos, head, data, ended = 8, None, [], False
    while pos < len(raw) and not ended:
        if pos + 12 > len(raw):
            raise ValueError("read_png: truncated chunk")
        n, tag = struct.unpack(">I4s", raw[pos:pos + 8])
        if pos + 12 + n > len(raw):
            raise ValueError("read_png: truncated chunk %r" % tag)
        body = raw[pos + 8:pos + 8 + n]
        if struct.unpack(">I", raw[pos + 8 + n:pos + 12 + n])[0] != zlib.crc32(tag + body) & 0xFFFFFFFF:
            raise ValueError("read_png: bad CRC in chunk %r" % tag)
        if head is None and tag != b"IHDR":
            raise ValueError("read_png: the first chunk is not IHDR")
        if tag == b"IHDR":
            if head is not None or n != 13:
                raise ValueError("read_png: bad IHDR")
            head = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            data.append(body)
        elif tag == b"IEND":
            ended = True
        elif not tag[0] & 0x20:                                # a critical chunk this reader does not know (PLTE among them)
            raise ValueError("read_png: unsupported critical chunk %r" % tag)
        pos += 12 + n
    if head is None or not ended:
        raise ValueError("read_png: no IHDR or no IEND")
    w, h, depth, colour, comp, filt, lace = head
    if depth != 8 or colour not in _PNG_CHANNELS or comp != 0 or filt != 0 or lace != 0 or w < 1 or h < 1:
        raise ValueError("read_png: only 8-bit grey, grey + alpha, RGB and RGBA, non-interlaced (got depth %d, colour type %d, "
                         "interlace %d)" % (depth, colour, lace))
    bpp = _PNG_CHANNELS[colour]
    stride = w * bpp
    try:
        flat = zlib.decompress(b"".join(data))
    except zlib.error as e:
        raise ValueError("read_png: %s" % e) from None
    if len(flat) != h * (1 + stride):
        raise ValueError("read_png: %d bytes of image data for %d x %d x %d" % (len(flat), h, w, bpp))
    lines = np.frombuffer(flat, dtype=np.uint8).reshape(h, 1 + stride)
    out = np.zeros((h, stride), dtype=np.uint8)
    prev = np.zeros(stride, dtype=np.int64)
    for y in range(h):
        kind, line = int(lines[y, 0]), lines[y, 1:].astype(np.int64)
        if kind == 0:
            cur = line
        elif kind == 2:                                        # Up
            cur = (line + prev) & 255
        elif kind in (1, 3, 4):                                # Sub, Average, Paeth: each byte needs the one bpp to its left
            cur = np.zeros(stride, dtype=np.int64)
            for x in range(stride):
                a = int(cur[x - bpp]) if x >= bpp else 0
                b = int(prev[x])
                if kind == 1:
                    pred = a
                elif kind == 3:
                    pred = (a + b) >> 1
                else:
                    c = int(prev[x - bpp]) if x >= bpp else 0
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                cur[x] = (int(line[x]) + pred) & 255
        else:
            raise ValueError("read_png: unknown filter type %d on line %d" % (kind, y))
        out[y] = cur
        prev = cur
    return out.reshape(h, w) if bpp == 1 else out.reshape(h, w, bpp)
