"""Host side of the dataset's image path: decoding an image file to 8-bit RGB (LLFF) or RGBA (Blender), and the
coefficient tables of Pillow's LANCZOS resize that the GPU passes (ops.data.resize_lanczos_u8, hn_resample_u8) apply.

Decoding uses Pillow when it imports (`Image.open(p).convert('RGB')`, what the reference's datasets/llff.py does);
without Pillow a PNG decoder of the standard library (zlib) reads 8-bit greyscale, grey+alpha, RGB and RGBA files with
any of the five scanline filters — slowly where a file uses the Average or Paeth filter (see `_unfilter`).  JPEG
without Pillow is refused.
"""
from __future__ import annotations

import math
import struct
import zlib
from typing import Tuple

import numpy as np

PRECISION_BITS = 22          # Pillow's 8-bit resampling: int32 coefficients with 32 - 8 - 2 fraction bits
LANCZOS_SUPPORT = 3.0

try:
    from PIL import Image as _PILImage
except ImportError:          # the package's own PNG decoder takes over
    _PILImage = None


def have_pillow() -> bool:
    return _PILImage is not None


# --------------------------------------------------------------------------------------------
# decoding
# --------------------------------------------------------------------------------------------
def load_rgb8(path: str, use_pillow: bool = True) -> np.ndarray:
    """An image file -> (H, W, 3) uint8 RGB."""
    if use_pillow and _PILImage is not None:
        with _PILImage.open(path) as im:
            return np.asarray(im.convert('RGB'), dtype=np.uint8).copy()
    with open(path, "rb") as f:
        data = f.read()
    if data[:8] == b"\x89PNG\r\n\x1a\n":
        return decode_png_rgb8(data)
    if data[:3] == b"\xff\xd8\xff":
        raise ValueError(f"{path}: JPEG images need Pillow, which is not installed (convert the images to PNG, or "
                         "install Pillow)")
    raise ValueError(f"{path}: not a PNG image, and Pillow is not installed to read other formats")


def load_rgba8(path: str, use_pillow: bool = True) -> np.ndarray:
    """An RGBA image file -> (H, W, 4) uint8, the bytes as stored (no mode conversion: the reference's Blender reader
    hands the opened image to ToTensor and fails in `img.view(4, -1)` on anything but four channels)."""
    if use_pillow and _PILImage is not None:
        with _PILImage.open(path) as im:
            if im.mode != 'RGBA':
                raise ValueError(f"{path}: the Blender dataset reads RGBA images (this one has mode '{im.mode}')")
            return np.asarray(im, dtype=np.uint8).copy()
    with open(path, "rb") as f:
        data = f.read()
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError(f"{path}: not a PNG image, and Pillow is not installed to read other formats")
    try:
        return decode_png_rgba8(data)
    except ValueError as e:
        raise ValueError(f"{path}: {e}") from None


def image_size(path: str, use_pillow: bool = True) -> Tuple[int, int]:
    """(width, height) of an image file from its header, without decoding the pixels."""
    if use_pillow and _PILImage is not None:
        with _PILImage.open(path) as im:
            return im.size
    with open(path, "rb") as f:
        head = f.read(24)
    if head[:8] == b"\x89PNG\r\n\x1a\n" and head[12:16] == b"IHDR":
        return struct.unpack(">II", head[16:24])
    return load_rgb8(path, use_pillow=False).shape[1::-1]       # raises the decoder's message


_CHANNELS = {0: 1, 2: 3, 4: 2, 6: 4}         # PNG colour type -> samples per pixel (8-bit types only)


def _unfilter(raw: bytes, h: int, stride: int, bpp: int) -> np.ndarray:
    """Undo the per-scanline filters (PNG spec §9): 0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth.  None, Sub and Up are
    NumPy per scanline; Average and Paeth depend on the reconstructed left neighbour and run byte by byte in Python —
    about a second per megabyte of such scanlines on one core, so a 12-megapixel photo (36 MB of samples) filtered
    that way takes about half a minute.  This path
    serves only installations without Pillow; with Pillow installed, images are decoded by Pillow."""
    rows = np.frombuffer(raw, dtype=np.uint8)
    if rows.size != h * (stride + 1):
        raise ValueError("PNG: image data has the wrong length")
    rows = rows.reshape(h, stride + 1)
    out = np.empty((h, stride), dtype=np.uint8)
    prev = np.zeros(stride, dtype=np.uint8)
    for y in range(h):
        ft, line = int(rows[y, 0]), rows[y, 1:]
        if ft == 0:
            cur = line.copy()
        elif ft == 1:        # Sub: a running sum per byte position within the pixel, mod 256
            cur = np.cumsum(line.reshape(-1, bpp), axis=0, dtype=np.uint8).reshape(-1)
        elif ft == 2:
            cur = line + prev
        elif ft in (3, 4):   # Average / Paeth: byte by byte, each depends on its reconstructed left neighbour
            f, b = line.tolist(), prev.tolist()
            c = [0] * stride
            for i in range(stride):
                a = c[i - bpp] if i >= bpp else 0
                if ft == 3:
                    c[i] = (f[i] + ((a + b[i]) >> 1)) & 0xff
                else:
                    ul = b[i - bpp] if i >= bpp else 0
                    p = a + b[i] - ul
                    pa, pb, pc = abs(p - a), abs(p - b[i]), abs(p - ul)
                    pred = a if (pa <= pb and pa <= pc) else (b[i] if pb <= pc else ul)
                    c[i] = (f[i] + pred) & 0xff
            cur = np.array(c, dtype=np.uint8)
        else:
            raise ValueError(f"PNG: unknown filter type {ft}")
        out[y] = cur
        prev = cur
    return out


def _decode_png(data: bytes) -> np.ndarray:
    """A PNG file's bytes -> (H, W, samples per pixel) uint8 as stored.  8 bits per sample, no interlace."""
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError("not a PNG")
    pos, idat, hdr = 8, [], None
    while pos + 12 <= len(data):
        n, tag = struct.unpack(">I", data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        if struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] != (zlib.crc32(tag + body) & 0xffffffff):
            raise ValueError("PNG chunk CRC mismatch")
        if tag == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body[:13])
        elif tag == b"IDAT":
            idat.append(body)
        elif tag == b"IEND":
            break
        pos += 12 + n
    if hdr is None:
        raise ValueError("PNG: no IHDR chunk")
    w, h, depth, colour, _, _, interlace = hdr
    if depth != 8 or colour not in _CHANNELS:
        raise ValueError(f"PNG: only 8-bit greyscale / RGB / RGBA images are read without Pillow (bit depth {depth}, "
                         f"colour type {colour})")
    if interlace:
        raise ValueError("PNG: interlaced images are read only with Pillow")
    ch = _CHANNELS[colour]
    return _unfilter(zlib.decompress(b"".join(idat)), h, w * ch, ch).reshape(h, w, ch)


def decode_png_rgb8(data: bytes) -> np.ndarray:
    """A PNG file's bytes -> (H, W, 3) uint8 RGB (alpha dropped, grey replicated: Pillow's convert('RGB') of those
    modes).  8 bits per sample, no interlace."""
    px = _decode_png(data)
    if px.shape[2] in (1, 2):
        return np.repeat(px[..., :1], 3, axis=2)
    return np.ascontiguousarray(px[..., :3])


def decode_png_rgba8(data: bytes) -> np.ndarray:
    """A PNG file's bytes -> (H, W, 4) uint8 RGBA, alpha kept.  Colour type 6 (8-bit RGBA) only: any other type is
    refused, as Pillow's mode of such a file is not 'RGBA'."""
    px = _decode_png(data)
    if px.shape[2] != 4:
        raise ValueError(f"PNG: the Blender dataset reads RGBA images (colour type 6); this one has {px.shape[2]} "
                         "sample(s) per pixel")
    return np.ascontiguousarray(px)


# --------------------------------------------------------------------------------------------
# LANCZOS coefficient tables (Pillow's precompute_coeffs + normalize_coeffs_8bpc, float64 host math)
# --------------------------------------------------------------------------------------------
def _sinc(x: float) -> float:
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x           # the C library's sin, as Pillow calls it (not NumPy's)


def _lanczos(x: float) -> float:
    if -LANCZOS_SUPPORT <= x < LANCZOS_SUPPORT:
        return _sinc(x) * _sinc(x / 3)
    return 0.0


def lanczos_weights(in_size: int, out_size: int):
    """Per output index: (first input index, float64 weights normalised to sum 1), for resampling an axis of length
    `in_size` to `out_size` over the whole input (box 0 .. in_size)."""
    scale = float(in_size) / out_size
    filterscale = max(scale, 1.0)
    support = LANCZOS_SUPPORT * filterscale
    ss = 1.0 / filterscale
    res = []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)          # int(): truncation toward zero, as C's cast
        hi = min(int(center + support + 0.5), in_size)
        ws = [_lanczos((x - center + 0.5) * ss) for x in range(lo, hi)]
        total = 0.0
        for v in ws:
            total += v
        if total != 0.0:
            ws = [v / total for v in ws]
        res.append((lo, ws))
    return res, int(math.ceil(support)) * 2 + 1


def lanczos_tables(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray, int]:
    """(bounds (out, 2) int32 [first, count], coefficients (out, ksize) int32 with 22 fraction bits, ksize): the tables
    of one hn_resample_u8 pass.  Rounding half away from zero."""
    weights, ksize = lanczos_weights(in_size, out_size)
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    kk = np.zeros((out_size, ksize), dtype=np.int32)
    one = float(1 << PRECISION_BITS)
    for xx, (lo, ws) in enumerate(weights):
        bounds[xx] = (lo, len(ws))
        for t, v in enumerate(ws):
            kk[xx, t] = int(-0.5 + v * one) if v < 0 else int(0.5 + v * one)
    return bounds, kk, ksize


def resample_u8_reference(img: np.ndarray, size) -> np.ndarray:
    """A NumPy statement of the two fixed-point passes hn_resample_u8 runs (tests): (H, W, C) uint8 -> (h, w, C)."""
    out_w, out_h = int(size[0]), int(size[1])
    x = np.asarray(img, dtype=np.uint8)

    def one_pass(a: np.ndarray, n_out: int, axis: int) -> np.ndarray:
        bounds, kk, _ = lanczos_tables(a.shape[axis], n_out)
        a = np.moveaxis(a, axis, 0).astype(np.int64)
        out = np.empty((n_out,) + a.shape[1:], dtype=np.uint8)
        for o in range(n_out):
            lo, n = bounds[o]
            acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(kk[o, :n].astype(np.int64), a[lo:lo + n], axes=(0, 0))
            acc = ((acc + (1 << 31)) % (1 << 32)) - (1 << 31)            # int32 wrap, as the device sums
            out[o] = np.clip(acc >> PRECISION_BITS, 0, 255)
        return np.moveaxis(out, 0, axis)

    if out_w != x.shape[1]:
        x = one_pass(x, out_w, 1)
    if out_h != x.shape[0]:
        x = one_pass(x, out_h, 0)
    return np.ascontiguousarray(x)


def premultiply_u8_reference(img: np.ndarray) -> np.ndarray:
    """Pillow's RGBA -> RGBa: c' = ((t >> 8) + t) >> 8 with t = c * a + 128; alpha unchanged."""
    x = np.asarray(img, dtype=np.uint8).astype(np.int64)
    t = x[..., :3] * x[..., 3:] + 128
    x[..., :3] = ((t >> 8) + t) >> 8
    return x.astype(np.uint8)


def unpremultiply_u8_reference(img: np.ndarray) -> np.ndarray:
    """Pillow's RGBa -> RGBA: the colour bytes stay where a is 0 or 255, else c = min(255, (255 * c') // a)."""
    x = np.asarray(img, dtype=np.uint8).astype(np.int64)
    a = x[..., 3:]
    x[..., :3] = np.where((a == 0) | (a == 255), x[..., :3], np.minimum(255, (255 * x[..., :3]) // np.maximum(a, 1)))
    return x.astype(np.uint8)


def resample_rgba8_reference(img: np.ndarray, size) -> np.ndarray:
    """A NumPy statement of ops.data.resize_lanczos_rgba8 (tests): Pillow's LANCZOS resize of an (H, W, 4) RGBA
    image — a copy at equal size, else premultiply, the two fixed-point passes on four channels, un-premultiply."""
    x = np.asarray(img, dtype=np.uint8)
    if x.ndim != 3 or x.shape[2] != 4:
        raise ValueError("resample_rgba8_reference: (H, W, 4) uint8")
    if (int(size[1]), int(size[0])) == x.shape[:2]:
        return x.copy()
    return unpremultiply_u8_reference(resample_u8_reference(premultiply_u8_reference(x), size))
