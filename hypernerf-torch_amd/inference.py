"""Evaluation-side drivers of the render path (reference: eval.py:77-101 `batched_inference`, the image assembly of
eval.py:139-166 and train.py:166-182).

`batched_inference` keeps the reference's signature and result (every per-level tensor concatenated over chunks).
`render_image` is what an MI355X wants instead: it keeps only the per-ray outputs an image needs (the (B,S,7) point
tensors the reference also concatenates are pure HBM traffic), uses chunks that fill the GPU, and shards the rays
of the image over the ranks of a data-parallel job (one all-gather of pixels, dist.all_gather_pixels).
"""
from __future__ import annotations

from collections import defaultdict
from typing import Dict, Sequence

import torch

from . import dist as hdist
from .hypernerf import model_utils
from .ops import gif

_EXTRA = {'nerf_alpha': None, 'warp_alpha': None, 'hyper_alpha': None, 'hyper_sheet_alpha': None}


@torch.no_grad()
def batched_inference(model, rays_dict, N_samples=None, N_importance=None, use_disp=False, chunk=1024 * 32,
                      white_back=False) -> Dict:
    """Render all rays of `rays_dict` in chunks of `chunk` rays and concatenate every output.  N_samples,
    N_importance, use_disp and white_back are accepted and ignored exactly as the reference ignores them (the model
    carries those settings); unlike the reference, `chunk` is honoured (eval.py:84 overwrites it with 1024)."""
    n = rays_dict["origins"].shape[0]
    pieces = defaultdict(list)
    for start in range(0, n, chunk):
        out = model(model_utils.extract_rays_batch(rays_dict, start, start + chunk), dict(_EXTRA))
        for level, tensors in out.items():
            pieces[level].append(tensors)
    return {level: model_utils.concat_ray_batch(chunks) for level, chunks in pieces.items()}


@torch.no_grad()
def render_image(model, rays: torch.Tensor, chunk: int = 16384, level: str = 'fine',
                 keys: Sequence[str] = ('rgb', 'depth', 'acc'), group=None, occupancy=None, near=None, far=None,
                 clip_far: bool = True, miss: str = 'render', miss_rgb=None) -> Dict[str, torch.Tensor]:
    """rays (N, 8|9) of one image -> {key: (N, ...)} for the requested per-ray outputs of `level`.
    With torch.distributed initialised every rank renders a contiguous 1/world slice and the pixels are gathered
    with one all-gather per key (slices are padded to equal length).

    `occupancy` (a dict of occupancy_grid / occupancy_from_density; None: everything below is off and the launches are
    today's) skips empty space: this rank's slice is clipped once (ops.occupancy.clip_rays) to the part
    of [near, far] between the first and the last occupied cell of each ray, the re-parametrised rows are rendered with
    the ORIGINAL directions as 'viewdirs' — the model spends its whole sample budget inside the clipped interval — and
    the results are mapped back to true distances (ops.occupancy.unclip: depth through the sum of the level's weights).
    `keys` may then hold 'rgb', 'depth', 'acc' and 'med_depth' only.  near / far: the interval the model samples,
    model.near / model.far by default; given explicitly they are also handed to the model's forward.
    clip_far: the interval ends at the exit of the last occupied cell, and the sample HyperNeRF treats as 'at infinity'
    (use_sample_at_infinity) then sits there, not at `far`; clip_far=False clips the front only and keeps it at `far`.
    miss='render' renders the rays that meet no occupied cell unclipped, exactly as without an occupancy; miss='skip'
    sends only the hit rays to the model and fills the others with rgb = miss_rgb (three floats or a float, default 0),
    depth, med_depth and acc 0: the caller asserts that there is nothing outside the grid.
    A lattice can miss structure thinner than a cell: sigma_min and dilate of the occupancy are the guard against that.
    A model with use_linear_disparity places its samples linearly in disparity of the re-parametrised z, i.e. over the
    clipped interval mapped onto [near, far], not in the disparity of the true distance."""
    if occupancy is not None or miss != 'render':
        from .ops import occupancy as occ_ops
        if miss not in ('render', 'skip'):
            raise ValueError(f"render_image: miss must be 'render' or 'skip', got {miss!r}")
        if occupancy is None:
            raise ValueError("render_image: miss='skip' needs an occupancy")
        unknown = [k for k in keys if k not in occ_ops.OCC_KEYS]
        if unknown:
            raise ValueError(f"render_image: with an occupancy the keys are {occ_ops.OCC_KEYS}, got {unknown}")
        fill = torch.as_tensor(0.0 if miss_rgb is None else miss_rgb, dtype=torch.float32).reshape(-1)
        if fill.numel() not in (1, 3):
            raise ValueError(f"render_image: miss_rgb must be a number or three numbers, got {miss_rgb!r}")
        model_kw = {k: float(v) for k, v in (('near', near), ('far', far)) if v is not None}
        t_near = model.near if near is None else near
        t_far = model.far if far is None else far
    n = rays.shape[0]
    world = torch.distributed.get_world_size(group) if hdist.dist.is_available() and hdist.dist.is_initialized() else 1
    rank = torch.distributed.get_rank(group) if world > 1 else 0
    lo, hi = hdist.shard_range(n, rank, world)
    per = -(-n // world)                                  # padded slice length, equal on all ranks
    mine = rays[lo:hi]
    outs = {k: [] for k in keys}
    if occupancy is None:
        for start in range(0, mine.shape[0], chunk):
            rd = model_utils.prepare_ray_dict(mine[start:start + chunk])
            res = model(rd, dict(_EXTRA))[level]
            for k in keys:
                outs[k].append(res[k])
    else:
        clip = occ_ops.clip_rays(mine, occupancy, t_near, t_far, clip_far=clip_far)
        rows, dirs, affine = clip['rays'], mine[:, 3:6], clip['affine']
        if miss == 'skip':
            kept = torch.nonzero(clip['hit']).reshape(-1)
            rows, dirs, affine = rows[kept], dirs[kept], affine[kept]
        need = [k for k in keys] + (['weights'] if 'depth' in keys else [])
        for start in range(0, rows.shape[0], chunk):
            rd = model_utils.prepare_ray_dict(rows[start:start + chunk])
            rd['viewdirs'] = dirs[start:start + chunk]
            res = model(rd, dict(_EXTRA), **model_kw)[level]
            res = occ_ops.unclip({k: res[k] for k in need}, affine[start:start + chunk])
            for k in keys:
                outs[k].append(res[k])
        if miss == 'skip':
            for k in keys:
                shape = (mine.shape[0], 3) if k == 'rgb' else (mine.shape[0],)
                full = torch.zeros(shape, dtype=torch.float32, device=rays.device)
                if k == 'rgb':
                    full[:] = fill.to(rays.device)
                if outs[k]:
                    got = torch.cat(outs[k], dim=0)
                    full[kept] = got.reshape((kept.shape[0],) + shape[1:]).to(full.dtype)
                outs[k] = [full] if mine.shape[0] else []
    result = {}
    for k in keys:
        if outs[k]:
            x = torch.cat(outs[k], dim=0)
        else:       # a rank without rays (more ranks than rays): shape from a zero-length template
            x = torch.zeros((0, 3) if k == 'rgb' else (0,), dtype=torch.float32, device=rays.device)
        if world > 1:
            pad = per - x.shape[0]
            if pad:
                x = torch.cat([x, x.new_zeros((pad,) + tuple(x.shape[1:]))], dim=0)
            full = hdist.all_gather_pixels(x, group)
            parts = []
            for r in range(world):
                a, b = hdist.shard_range(n, r, world)
                parts.append(full[r * per:r * per + (b - a)])
            x = torch.cat(parts, dim=0)
        result[k] = x
    return result


def write_png(path: str, img8) -> None:
    """8-bit RGB (H, W, 3) uint8 array / tensor -> a PNG file, with the standard library only (zlib + struct): what
    eval.py:166 does through imageio (`imageio.imwrite(f'{i:03d}.png', img_pred_)`), without an image library in the
    package's dependencies.  Truecolour, 8 bits per channel, no interlace, filter type 0 on every scanline."""
    import struct
    import zlib
    import numpy as np
    a = np.ascontiguousarray(img8.cpu().numpy() if isinstance(img8, torch.Tensor) else img8, dtype=np.uint8)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("write_png: (H, W, 3) uint8")
    h, w = a.shape[:2]
    raw = np.concatenate([np.zeros((h, 1), dtype=np.uint8), a.reshape(h, w * 3)], axis=1).tobytes()      # filter byte 0 per row

    def chunk(tag: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def read_png(path: str):
    """The inverse of write_png for its own files (tests): (H, W, 3) uint8 numpy array."""
    import struct
    import zlib
    import numpy as np
    data = open(path, "rb").read()
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError("not a PNG")
    pos, idat, w, h = 8, b"", 0, 0
    while pos < len(data):
        n, tag = struct.unpack(">I", data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        if struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] != (zlib.crc32(tag + body) & 0xffffffff):
            raise ValueError("PNG chunk CRC mismatch")
        if tag == b"IHDR":
            w, h, depth, colour = struct.unpack(">IIBB", body[:10])
            if (depth, colour) != (8, 2):
                raise ValueError("read_png reads 8-bit truecolour only")
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    rows = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, 1 + 3 * w)
    if rows[:, 0].any():
        raise ValueError("read_png reads filter type 0 only")
    return rows[:, 1:].reshape(h, w, 3).copy()


def write_pfm(path: str, image, scale: float = 1) -> None:
    """float32 (H, W), (H, W, 1) or (H, W, 3) array / tensor -> a PFM file, byte for byte what the reference's save_pfm
    writes (datasets/depth_utils.py:43-69): 'Pf' (greyscale) or 'PF' (colour), 'W H', the scale negated on a
    little-endian array ('%f', so '-1.000000'), then the rows bottom to top.  numpy and the standard library only."""
    import sys
    import numpy as np
    a = image.detach().cpu().numpy() if isinstance(image, torch.Tensor) else np.asarray(image)
    if a.dtype.name != "float32":          # either byte order
        raise ValueError("write_pfm: the image must be float32")
    if a.ndim == 3 and a.shape[2] == 3:
        color = True
    elif a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 1):
        color = False
    else:
        raise ValueError("write_pfm: (H, W), (H, W, 1) or (H, W, 3)")
    a = np.flipud(a)
    endian = a.dtype.byteorder
    if endian == '<' or (endian == '=' and sys.byteorder == 'little'):
        scale = -scale
    with open(path, "wb") as f:
        f.write(b"PF\n" if color else b"Pf\n")
        f.write(f"{a.shape[1]} {a.shape[0]}\n".encode())
        f.write(("%f\n" % scale).encode())
        a.tofile(f)


def read_pfm(path: str):
    """A PFM file -> (data, scale) as the reference's read_pfm returns them (datasets/depth_utils.py:5-40): (H, W) for
    'Pf', (H, W, 3) for 'PF', either endianness (a negative scale marks little-endian; the scale comes back positive),
    rows top to bottom."""
    import re
    import numpy as np
    with open(path, "rb") as f:
        header = f.readline().decode("utf-8").rstrip()
        if header not in ("PF", "Pf"):
            raise ValueError("not a PFM file")
        color = header == "PF"
        dims = re.match(r"^(\d+)\s(\d+)\s$", f.readline().decode("utf-8"))
        if dims is None:
            raise ValueError("malformed PFM header")
        width, height = map(int, dims.groups())
        scale = float(f.readline().rstrip())
        endian = "<" if scale < 0 else ">"
        scale = abs(scale)
        data = np.fromfile(f, endian + "f")
    data = data.reshape((height, width, 3) if color else (height, width))
    return np.flipud(data), scale


# ------------------------------------------------------------------------------------------------------------------
# The GIF of the evaluated frames (eval.py:172, imageio.mimsave(..., fps=30)).  A GIF colour table has at most 256
# entries: the frames are quantised on the device (ops.gif.color_histogram / palette_map), the palette is cut on the
# host from the 2^18-cell table, the index maps are LZW-coded by the library's host code (ops.gif.gif_lzw) and the
# container is written with the standard library.
# ------------------------------------------------------------------------------------------------------------------
GIF_COLORS = 256


def palette_from_histogram(hist, colors: int = GIF_COLORS):
    """(palette (256, 3) uint8 array, n_colors) from a colour table of ops.gif.color_histogram: a pure, deterministic
    function of the table (`colors`: fewer boxes than a GIF table holds, 1..256).  Entries are its non-empty cells: key k, count c, mean colour sums / c in float64.  With at
    most 256 entries the palette is floor(mean + 0.5) of each, in key order.  Otherwise median cut: one box holds all
    entries; until there are 256 boxes the box with more than one entry and the largest count_sum * range is cut (range:
    the largest per-channel extent of its entries' means; equal scores: the lower box index, equal extents: the lower
    channel), its entries ordered by (mean on that channel, key), after the first entry whose cumulative count reaches
    half of the box's count (both sides keep at least one entry); the left part keeps the box's index, the right part
    is appended.  A palette entry is floor(sum of sums / sum of counts + 0.5) of its box; unused entries are zero.
    The scores of untouched boxes are kept from cut to cut, so a frame with 3e4 cells costs 255 small sorts."""
    import numpy as np
    h = np.asarray(hist.detach().cpu().numpy() if isinstance(hist, torch.Tensor) else hist)
    if h.ndim != 2 or h.shape[1] != 4 or h.dtype.kind not in "iu":
        raise ValueError("palette_from_histogram: an (N, 4) integer table [count, sum r, sum g, sum b]")
    h = h.astype(np.int64, copy=False)
    keys = np.flatnonzero(h[:, 0])
    if keys.size == 0:
        raise ValueError("palette_from_histogram: the table is empty")
    if not 1 <= colors <= GIF_COLORS:
        raise ValueError("palette_from_histogram: 1 .. 256 colours")
    cnt, sums = h[keys, 0], h[keys, 1:4]
    means = sums / cnt[:, None].astype(np.float64)
    pal = np.zeros((GIF_COLORS, 3), dtype=np.uint8)
    if keys.size <= colors:
        pal[:keys.size] = np.floor(means + 0.5).astype(np.uint8)
        return pal, int(keys.size)

    def score(idx):
        if idx.size < 2:
            return -1.0, 0
        m = means[idx]
        ext = m.max(axis=0) - m.min(axis=0)
        ch = int(np.argmax(ext))                        # the first maximum: the lower channel
        return float(int(cnt[idx].sum())) * float(ext[ch]), ch

    boxes = [np.arange(keys.size)]
    scored = [score(boxes[0])]
    while len(boxes) < colors:
        b = int(np.argmax([s for s, _ in scored]))      # the first maximum: the lower box index
        idx, ch = boxes[b], scored[b][1]
        idx = idx[np.lexsort((keys[idx], means[idx, ch]))]
        cum = np.cumsum(cnt[idx])
        j = min(int(np.searchsorted(2 * cum, cum[-1], side="left")), idx.size - 2)
        boxes[b], right = idx[:j + 1], idx[j + 1:]
        boxes.append(right)
        scored[b] = score(boxes[b])
        scored.append(score(right))
    for b, idx in enumerate(boxes):
        pal[b] = np.floor(sums[idx].sum(axis=0) / float(int(cnt[idx].sum())) + 0.5).astype(np.uint8)
    return pal, colors


def _check_frames(frames, what: str):
    """A non-empty list of equally sized (H, W, 3) uint8 frames as tensors; ValueError otherwise."""
    import numpy as np
    if isinstance(frames, (torch.Tensor, np.ndarray)) and frames.ndim == 4:
        frames = list(frames)
    frames = [torch.from_numpy(np.ascontiguousarray(f)) if isinstance(f, np.ndarray) else f for f in frames]
    if not frames:
        raise ValueError(f"{what}: no frames")
    for f in frames:
        if not isinstance(f, torch.Tensor) or f.dtype != torch.uint8 or f.dim() != 3 or f.shape[2] != 3:
            raise ValueError(f"{what}: every frame must be (H, W, 3) uint8")
        if f.shape != frames[0].shape:
            raise ValueError(f"{what}: frames differ in size: {tuple(f.shape[:2])} and {tuple(frames[0].shape[:2])}")
    _check_gif_size(int(frames[0].shape[0]), int(frames[0].shape[1]), what)
    return frames


def _check_gif_size(h: int, w: int, what: str):
    if not (1 <= h <= 65535 and 1 <= w <= 65535):
        raise ValueError(f"{what}: a GIF side is 1 .. 65535 pixels, got {h} x {w}")


@torch.no_grad()
def quantize_frames(frames, palette: str = "global"):
    """(palettes, indices) of uint8 (H, W, 3) frames, on the device or the host (host frames are uploaded: the colour
    table and the palette search run in HIP, and there is no CPU fallback).  palette='global': ONE colour table over all
    frames and one palette, so a colour keeps its index from frame to frame and nothing flickers; 'frame': one palette
    per frame.  palettes: a list (of one, or one per frame) of (256, 3) uint8 host tensors, unused entries zero;
    indices: one (H, W) uint8 host tensor per frame, each pixel the nearest USED palette entry (squared RGB distance,
    the smaller index among equals).  No dithering."""
    from . import _lib as L
    if palette not in ("global", "frame"):
        raise ValueError("palette: 'global' or 'frame'")
    frames = _check_frames(frames, "quantize_frames")
    dev = next((f.device for f in frames if f.is_cuda), None)
    if dev is None:
        if not torch.cuda.is_available():
            L.require_gpu(frames[0])
        dev = torch.device("cuda", torch.cuda.current_device())
    frames = [f.to(dev).contiguous() for f in frames]
    palettes, indices = [], []
    if palette == "global":
        table = None
        for f in frames:
            table = gif.color_histogram(f, out=table)
        pal, n_colors = palette_from_histogram(table)
        palettes.append(torch.from_numpy(pal))
        pal_dev = palettes[0][:n_colors].to(dev)
        indices = [gif.palette_map(f, pal_dev).cpu() for f in frames]
    else:
        for f in frames:
            pal, n_colors = palette_from_histogram(gif.color_histogram(f))
            palettes.append(torch.from_numpy(pal))
            indices.append(gif.palette_map(f, palettes[-1][:n_colors].to(dev)).cpu())
    return palettes, indices


def write_gif(path: str, frames, fps: float = 30, loop: int = 0, palette: str = "global") -> None:
    """Frames -> an animated GIF, what eval.py:172 does through imageio (`imageio.mimsave(..., fps=30)`), with the
    standard library only.  `frames`: uint8 (H, W, 3) frames (quantised by `quantize_frames(frames, palette)`, on the
    GPU), or the (palettes, indices) pair quantize_frames returned (one palette for 'global', one per frame for
    'frame').  Layout: 'GIF89a'; the logical screen; for 'global' a global colour table, for 'frame' a local table in
    front of every image, always 256 entries; the NETSCAPE2.0 application block with `loop` repetitions (0 = for ever);
    per frame a graphic control extension with the delay max(1, round(100 / fps)) centiseconds (fps=30 gives 3, as
    imageio and Pillow write it), no disposal, no transparency; an image descriptor covering the whole screen; LZW
    minimum code size 8 and the code bytes of ops.gif.gif_lzw in sub-blocks of at most 255.  ValueError: no frames,
    frames of differing size, a side above 65535."""
    import struct
    if palette not in ("global", "frame"):
        raise ValueError("palette: 'global' or 'frame'")
    if not fps > 0:
        raise ValueError("fps must be positive")
    if not 0 <= int(loop) <= 65535:
        raise ValueError("loop: 0 .. 65535")
    if isinstance(frames, tuple) and len(frames) == 2 and isinstance(frames[0], (list, tuple)):
        palettes, indices = list(frames[0]), list(frames[1])
        if not indices:
            raise ValueError("write_gif: no frames")
        indices = [torch.as_tensor(x) for x in indices]
        palettes = [torch.as_tensor(p) for p in palettes]
        for x in indices:
            if x.dtype != torch.uint8 or x.dim() != 2:
                raise ValueError("write_gif: every index map must be (H, W) uint8")
            if x.shape != indices[0].shape:
                raise ValueError(f"write_gif: frames differ in size: {tuple(x.shape)} and {tuple(indices[0].shape)}")
        for p in palettes:
            if p.dtype != torch.uint8 or tuple(p.shape) != (GIF_COLORS, 3):
                raise ValueError("write_gif: every palette must be (256, 3) uint8")
        if len(palettes) != (1 if palette == "global" else len(indices)):
            raise ValueError(f"write_gif: palette='{palette}' with {len(palettes)} palettes for {len(indices)} frames")
        _check_gif_size(int(indices[0].shape[0]), int(indices[0].shape[1]), "write_gif")
    else:
        palettes, indices = quantize_frames(_check_frames(frames, "write_gif"), palette)
    h, w = (int(s) for s in indices[0].shape)
    delay = max(1, int(round(100.0 / fps)))
    if delay > 65535:
        raise ValueError("fps: the delay of a frame is at most 65535 centiseconds")

    def table(p) -> bytes:
        return p.cpu().contiguous().numpy().tobytes()
    out = [b"GIF89a", struct.pack("<HHBBB", w, h, 0xF7 if palette == "global" else 0x70, 0, 0)]
    if palette == "global":
        out.append(table(palettes[0]))
    out.append(b"\x21\xff\x0bNETSCAPE2.0\x03\x01" + struct.pack("<H", int(loop)) + b"\x00")
    for i, idx in enumerate(indices):
        out.append(b"\x21\xf9\x04\x00" + struct.pack("<H", delay) + b"\x00\x00")
        out.append(b"\x2c" + struct.pack("<HHHHB", 0, 0, w, h, 0x00 if palette == "global" else 0x87))
        if palette == "frame":
            out.append(table(palettes[i]))
        codes = gif.gif_lzw(idx.cpu().contiguous())
        out.append(b"\x08")
        out.extend(bytes([len(codes[s:s + 255])]) + codes[s:s + 255] for s in range(0, len(codes), 255))
        out.append(b"\x00")
    out.append(b"\x3b")
    with open(path, "wb") as f:
        f.write(b"".join(out))


def _gif_lzw_decode(data: bytes, min_code: int) -> bytes:
    clear, end = 1 << min_code, (1 << min_code) + 1
    table, prev, width = None, None, min_code + 1
    out = bytearray()
    acc = bits = pos = 0
    while True:
        while bits < width:
            if pos >= len(data):
                raise ValueError("GIF: the LZW stream ends without an end code")
            acc |= data[pos] << bits
            pos += 1
            bits += 8
        code = acc & ((1 << width) - 1)
        acc >>= width
        bits -= width
        if code == clear:
            table = [bytes([i]) for i in range(clear)] + [b"", b""]
            prev, width = None, min_code + 1
            continue
        if code == end:
            return bytes(out)
        if table is None:
            raise ValueError("GIF: the LZW stream does not open with a clear code")
        if prev is None:
            if code >= clear:
                raise ValueError("GIF: bad first LZW code")
            entry = table[code]
        else:
            if code < len(table):
                entry = table[code]
            elif code == len(table) and len(table) < 4096:
                entry = prev + prev[:1]
            else:
                raise ValueError("GIF: LZW code outside the table")
            if len(table) < 4096:
                table.append(prev + entry[:1])
        if len(table) == (1 << width) and width < 12:
            width += 1
        out += entry
        prev = entry


def read_gif(path: str):
    """The inverse of write_gif (tests; the standard library and numpy): {'frames': [(H, W, 3) uint8 arrays],
    'delays_cs': [centiseconds per frame], 'loop': the NETSCAPE2.0 repetition count or None}.  Reads what write_gif
    writes and a little more: global or local colour tables of any size, images smaller than the screen (drawn over the
    previous frame), any LZW minimum code size; no interlace, no transparency handling."""
    import struct
    import numpy as np
    data = open(path, "rb").read()
    if data[:6] not in (b"GIF89a", b"GIF87a"):
        raise ValueError("not a GIF")
    w, h, packed = struct.unpack("<HHB", data[6:11])
    pos, gct = 13, None
    if packed & 0x80:
        n = 3 << ((packed & 7) + 1)
        gct = np.frombuffer(data[pos:pos + n], dtype=np.uint8).reshape(-1, 3)
        pos += n

    def sub_blocks(pos):
        parts = []
        while data[pos]:
            parts.append(data[pos + 1:pos + 1 + data[pos]])
            pos += 1 + data[pos]
        return b"".join(parts), pos + 1
    frames, delays, loop, delay = [], [], None, 0
    canvas = np.zeros((h, w, 3), dtype=np.uint8)
    while True:
        tag = data[pos]
        if tag == 0x3B:
            break
        if tag == 0x21:
            label = data[pos + 1]
            body, end = sub_blocks(pos + 2)
            if label == 0xF9:
                delay = struct.unpack("<H", body[1:3])[0]
            elif label == 0xFF and body[:11] == b"NETSCAPE2.0" and body[11:12] == b"\x01":
                loop = struct.unpack("<H", body[12:14])[0]
            pos = end
        elif tag == 0x2C:
            x0, y0, fw, fh, fpacked = struct.unpack("<HHHHB", data[pos + 1:pos + 10])
            pos += 10
            if fpacked & 0x40:
                raise ValueError("read_gif does not read interlaced images")
            table = gct
            if fpacked & 0x80:
                n = 3 << ((fpacked & 7) + 1)
                table = np.frombuffer(data[pos:pos + n], dtype=np.uint8).reshape(-1, 3)
                pos += n
            if table is None:
                raise ValueError("GIF: an image without a colour table")
            min_code = data[pos]
            codes, pos = sub_blocks(pos + 1)
            idx = np.frombuffer(_gif_lzw_decode(codes, min_code), dtype=np.uint8)
            if idx.size != fw * fh or x0 + fw > w or y0 + fh > h:
                raise ValueError("GIF: an image does not match its descriptor")
            if idx.size and int(idx.max()) >= table.shape[0]:
                raise ValueError("GIF: an index outside the colour table")
            canvas[y0:y0 + fh, x0:x0 + fw] = table[idx].reshape(fh, fw, 3)
            frames.append(canvas.copy())
            delays.append(delay)
        else:
            raise ValueError(f"GIF: unknown block 0x{tag:02x}")
    return {"frames": frames, "delays_cs": delays, "loop": loop}


# ------------------------------------------------------------------------------------------------------------------
# The depth image and the image stack of the validation step (utils/visualization.py:6-18, train.py:175-183)
# ------------------------------------------------------------------------------------------------------------------
def jet_lut() -> torch.Tensor:
    """(256, 3) uint8 colour table for visualize_depth, BLUE channel first: the reference hands OpenCV's BGR array of
    cv2.applyColorMap(x, COLORMAP_JET) to Image.fromarray unswapped, so channel 0 of its picture is cv2's blue.  The table
    is MATLAB's jet(64) — per channel a trapezoid in sixteenths: red 0 up to entry 24, rising 1/16 .. 1 over entries
    24..39, 1 to entry 54, falling to 8/16 at entry 63; green the 47-entry trapezoid from entry 8; blue 9/16 rising to 1
    at entry 7, 1 to entry 22, falling to 1/16 at entry 38, 0 after — interpolated linearly from 64 to 256 entries and
    times 255, rounded to nearest (halves to even), which is how OpenCV states its JET table.  Integer arithmetic: entry
    k sits at 63 k / 255 = 21 k / 85 on the 64-entry axis."""
    u = list(range(1, 17)) + [16] * 15 + list(range(16, 0, -1))
    red, green, blue = [0] * 64, [0] * 64, [0] * 64
    red[24:64] = u[0:40]
    green[8:55] = u
    blue[0:39] = u[8:47]
    lut = torch.zeros((256, 3), dtype=torch.uint8)
    for c, chan in enumerate((blue, green, red)):
        for k in range(256):
            i, m = divmod(21 * k, 85)
            a, b = chan[i], chan[min(i + 1, 63)]
            q, r = divmod(3 * (85 * a + (b - a) * m), 16)          # 255 * value = 3 * (85 a + (b - a) m) / 16
            lut[k, c] = q + (1 if 2 * r > 16 or (2 * r == 16 and q % 2 == 1) else 0)
    return lut


def _unit_u8(device) -> torch.Tensor:
    """k / 255 in float32 for k = 0..255, divided (not multiplied by a reciprocal) on the host: ToTensor's values."""
    import numpy as np
    return torch.from_numpy(np.arange(256, dtype=np.float32) / np.float32(255)).to(device)


@torch.no_grad()
def visualize_depth(depth: torch.Tensor, lut=None) -> torch.Tensor:
    """(H, W) depth on the device -> the (3, H, W) float32 picture of utils/visualization.py:visualize_depth, on the
    device: nan_to_num, min-max normalisation, (255 x).astype(uint8), the colour table (ops.gif.depth_colormap: HIP,
    no host read) and ToTensor's uint8 / 255.  `lut`: a (256, 3) uint8 table, jet_lut() by default."""
    if not isinstance(depth, torch.Tensor) or depth.dim() != 2:
        raise ValueError("visualize_depth: depth must be an (H, W) tensor")
    img8 = gif.depth_colormap(depth.detach().float(), jet_lut() if lut is None else lut)
    return _unit_u8(img8.device)[img8.long()].permute(2, 0, 1).contiguous()


@torch.no_grad()
def validation_stack(gt: torch.Tensor, pred: torch.Tensor, depth: torch.Tensor, lut=None) -> torch.Tensor:
    """The (3, 3, H, W) stack [ground truth, prediction, depth picture] the validation step logs (train.py:175-183), on
    the host as there.  gt, pred: (H, W, 3) or (H*W, 3) images in [0, 1]; depth: the (H, W) depth map (coloured by
    visualize_depth, on the GPU) or an already coloured (3, H, W) picture."""
    if depth.dim() == 2:
        depth = visualize_depth(depth, lut)
    if depth.dim() != 3 or depth.shape[0] != 3:
        raise ValueError("validation_stack: depth must be (H, W) or a (3, H, W) picture")
    h, w = int(depth.shape[1]), int(depth.shape[2])
    planes = []
    for name, img in (("gt", gt), ("pred", pred)):
        if img.shape[-1] != 3 or img.numel() != h * w * 3:
            raise ValueError(f"validation_stack: {name} must be ({h}, {w}, 3) or ({h * w}, 3)")
        planes.append(img.detach().reshape(h, w, 3).permute(2, 0, 1).float().cpu())
    return torch.stack(planes + [depth.float().cpu()])


def _image_occupancy(occupancy, rays: torch.Tensor, i: int):
    """The occupancy dict of image i: `occupancy` itself, or an OccupancyCache's grid of the frame in column 8 of the rays."""
    from .ops.occupancy import OccupancyCache
    if not isinstance(occupancy, OccupancyCache):
        return occupancy
    if rays.dim() != 2 or rays.shape[1] < 9:
        raise ValueError(f"evaluate_images: an OccupancyCache needs the frame id in column 8 of the rays; image {i} has "
                         f"rays of shape {tuple(rays.shape)}")
    if rays.shape[0] == 0:
        raise ValueError(f"evaluate_images: image {i} has no rays to read a frame id from")
    first, last = (float(v) for v in torch.stack([rays[:, 8].min(), rays[:, 8].max()]).tolist())      # one host read
    if first != last or first != int(first):
        raise ValueError(f"evaluate_images: image {i} holds frame ids {first} .. {last}; an OccupancyCache needs one "
                         "integer id per image")
    return occupancy.get(int(first))


@torch.no_grad()
def evaluate_images(model, images, chunk: int = 16384, white_back: bool = False, save_dir=None, group=None,
                    image_format: str = "png", save_depth: bool = False, depth_format: str = "pfm",
                    use_valid_mask: bool = False, ms_ssim: bool = False, save_gif=None, gif_fps: float = 30,
                    gif_palette: str = "global", save_depth_gif: bool = False, lpips=None, occupancy=None,
                    clip_far: bool = True) -> Dict:
    """The per-image loop of the reference's eval.py:145-178 on the GPU: for every sample {'rays': (H*W, 8|9),
    'rgbs': (H*W, 3) optional, 'hw': (H, W) optional} render the fine level in chunks, form the (H, W, 3) image,
    its 8-bit version (eval.py:165 `(img*255).astype(uint8)`) and, when ground truth is present, the PSNR
    (metrics.psnr, eval.py:169-172) and the SSIM (metrics.ssim on (1, 3, H, W) views, no copy).  Returns
    {'images': [uint8 (H,W,3) CPU tensors], 'depths': [...], 'psnrs': [float], 'mean_psnr': float | None,
    'ssims': [float], 'mean_ssim': float | None}.  With `save_dir` the 8-bit frames are also written as `{i:03d}.png`
    (eval.py:166; `write_png`: standard library only — round 6; `image_format="ppm"` keeps the binary PPM of rounds 2-5).
    `save_depth` writes every depth map (after nan_to_num) into `save_dir` (eval.py:150-158): `depth_{i:03d}.pfm`
    (`write_pfm`, the reference's save_pfm layout) for depth_format 'pfm', the raw float32 bytes as `depth_{i:03d}` for
    'bytes' — the reference writes that file into the current directory (eval.py:157), this port into `save_dir`.
    `save_gif='scene'` writes the reference's GIF of all frames (eval.py:172, imageio.mimsave(..., fps=30)) as
    `save_dir/scene.gif` from the 8-bit frames formed here, quantised on the device (`write_gif` with `gif_fps` and
    `gif_palette`); `save_depth_gif` writes the colour-mapped depths (ops.gif.depth_colormap with jet_lut(), the
    picture of visualize_depth) as `scene_depth.gif` (`depth.gif` without `save_gif`).  Both need `save_dir`; without
    them the files written, the result and the work done are unchanged.
    `white_back` is accepted and ignored as in the reference's batched_inference (eval.py:77-85).
    `use_valid_mask` restricts the PSNR to the sample's 'valid_mask' ((H*W,) bool; the Blender splits carry alpha > 0)
    through metrics.psnr's own argument; off by default, as the reference's eval.py does not mask.
    `ms_ssim` adds the multi-scale SSIM (losses.ms_ssim, the metric of the published Nerfies / HyperNeRF tables) of every
    image with ground truth, on the same views as the SSIM: the result then also has 'ms_ssims': [float] and
    'mean_ms_ssim': float | None.  Off by default: the result and the work done are unchanged.
    `lpips` = an LpipsWeights (losses.load_lpips) on the model's device adds LPIPS (losses.lpips) the same way, on the same
    views: 'lpips': [float] and 'mean_lpips': float | None.  None by default: the result and the work done are unchanged.
    `occupancy` skips empty space in every image (render_image's `occupancy` and `clip_far`; missed rays are rendered
    unclipped): an occupancy dict serves all images; an ops.occupancy.OccupancyCache gives each image the grid of its
    frame, the id in column 8 of its rays, which must be one value per image (8-column rays are refused).  A model
    trained with use_sample_at_infinity has learnt the colour of its last sample at `far`: clip_far=False keeps it there
    (DESIGN.md 3.18 has the measurement).  None by default: the result and the work done are unchanged."""
    if image_format not in ("png", "ppm"):
        raise ValueError("image_format: 'png' or 'ppm'")
    if depth_format not in ("pfm", "bytes"):
        raise ValueError("depth_format: 'pfm' or 'bytes'")
    if save_depth and save_dir is None:
        raise ValueError("save_depth needs save_dir")
    if (save_gif is not None or save_depth_gif) and save_dir is None:
        raise ValueError("save_gif / save_depth_gif need save_dir")
    if gif_palette not in ("global", "frame"):
        raise ValueError("gif_palette: 'global' or 'frame'")
    from .losses import psnr as _psnr
    from .losses import ssim as _ssim
    from .losses import ms_ssim as _ms_ssim
    from .losses import lpips as _lpips
    imgs, depths, psnrs, ssims, ms_ssims, lpipss = [], [], [], [], [], []
    gif_frames, depth_frames = [], []
    if save_depth_gif:
        lut = jet_lut()
    for i, sample in enumerate(images):
        rays = sample['rays']
        if occupancy is None:
            res = render_image(model, rays, chunk=chunk, keys=('rgb', 'depth'), group=group)
        else:
            res = render_image(model, rays, chunk=chunk, keys=('rgb', 'depth'), group=group,
                               occupancy=_image_occupancy(occupancy, rays, i), clip_far=clip_far)
        n = rays.shape[0]
        h, w = sample.get('hw', (1, n))
        img = res['rgb'].view(h, w, 3)
        img8_dev = (img * 255).to(torch.uint8)            # truncation, like numpy's astype(uint8) on [0, 1] data
        img8 = img8_dev.cpu()
        imgs.append(img8)
        if save_gif is not None:
            gif_frames.append(img8_dev)
        if save_depth_gif:
            depth_frames.append(gif.depth_colormap(res['depth'].view(h, w).float(), lut))
        depths.append(torch.nan_to_num(res['depth'].view(h, w)).cpu())
        if sample.get('rgbs') is not None:
            gt = sample['rgbs'].to(img.device).view(h, w, 3)
            mask = sample.get('valid_mask') if use_valid_mask else None
            psnrs.append(float(_psnr(gt, img, None if mask is None else mask.to(img.device).view(h, w))))
            ssims.append(float(_ssim(img.permute(2, 0, 1)[None], gt.permute(2, 0, 1)[None])))
            if ms_ssim:
                ms_ssims.append(float(_ms_ssim(img.permute(2, 0, 1)[None], gt.permute(2, 0, 1)[None])))
            if lpips is not None:
                lpipss.append(float(_lpips(img.permute(2, 0, 1)[None], gt.permute(2, 0, 1)[None], lpips)))
        if save_dir is not None:
            import os
            os.makedirs(save_dir, exist_ok=True)
            if save_depth:
                if depth_format == "pfm":
                    write_pfm(os.path.join(save_dir, f"depth_{i:03d}.pfm"), depths[-1].numpy())
                else:
                    with open(os.path.join(save_dir, f"depth_{i:03d}"), "wb") as f:
                        f.write(depths[-1].numpy().tobytes())
            if image_format == "png":
                write_png(os.path.join(save_dir, f"{i:03d}.png"), img8)
            else:
                with open(os.path.join(save_dir, f"{i:03d}.ppm"), "wb") as f:
                    f.write(f"P6 {w} {h} 255\n".encode() + img8.numpy().tobytes())
    if save_dir is not None and (gif_frames or depth_frames):
        import os
        if gif_frames:
            write_gif(os.path.join(save_dir, f"{save_gif}.gif"), gif_frames, fps=gif_fps, palette=gif_palette)
        if depth_frames:
            name = f"{save_gif}_depth.gif" if save_gif is not None else "depth.gif"
            write_gif(os.path.join(save_dir, name), depth_frames, fps=gif_fps, palette=gif_palette)
    out = {'images': imgs, 'depths': depths, 'psnrs': psnrs,
           'mean_psnr': (sum(psnrs) / len(psnrs)) if psnrs else None,
           'ssims': ssims, 'mean_ssim': (sum(ssims) / len(ssims)) if ssims else None}
    if ms_ssim:
        out['ms_ssims'] = ms_ssims
        out['mean_ms_ssim'] = (sum(ms_ssims) / len(ms_ssims)) if ms_ssims else None
    if lpips is not None:
        out['lpips'] = lpipss
        out['mean_lpips'] = (sum(lpipss) / len(lpipss)) if lpipss else None
    return out
