"""NumPy / pure-Python statements of the GIF path (csrc/hn_gif.hip, inference.quantize_frames / write_gif /
visualize_depth): the 2^18-cell colour table, the median cut over it, the nearest-of-K map with its tie rule, the depth
colour map in float32, and an LZW coder and decoder written independently of the library's (dictionaries of byte
strings, no hash table, no shared code).  Test infrastructure only."""
import numpy as np

HIST_BINS = 1 << 18


def keys_of(pixels):
    p = np.asarray(pixels, dtype=np.uint8).reshape(-1, 3).astype(np.int64)
    return ((p[:, 0] >> 2) << 12) | ((p[:, 1] >> 2) << 6) | (p[:, 2] >> 2)


def color_histogram(pixels, out=None):
    """(2^18, 4) int64: [count, sum r, sum g, sum b] per cell; adds to `out` when given."""
    p = np.asarray(pixels, dtype=np.uint8).reshape(-1, 3).astype(np.int64)
    k = keys_of(p)
    h = np.zeros((HIST_BINS, 4), dtype=np.int64) if out is None else out
    np.add.at(h[:, 0], k, 1)
    for c in range(3):
        np.add.at(h[:, 1 + c], k, p[:, c])
    return h


def median_cut(hist, colors=256):
    """(palette (colors, 3) uint8, n_used): the definition of inference.palette_from_histogram, as a plain loop that
    scores every box anew at every cut."""
    h = np.asarray(hist, dtype=np.int64)
    entries = [(int(k), int(h[k, 0]), tuple(int(v) for v in h[k, 1:4])) for k in np.flatnonzero(h[:, 0])]
    mean = {k: tuple(s / c for s in sums) for k, c, sums in entries}           # float64 divisions
    pal = np.zeros((colors, 3), dtype=np.uint8)
    if len(entries) <= colors:
        for i, (k, c, sums) in enumerate(entries):
            pal[i] = [int(np.floor(m + 0.5)) for m in mean[k]]
        return pal, len(entries)
    boxes = [entries]
    while len(boxes) < colors:
        best, best_score, best_ch = None, None, None
        for b, box in enumerate(boxes):
            if len(box) < 2:
                continue
            ext = [max(mean[k][ch] for k, _, _ in box) - min(mean[k][ch] for k, _, _ in box) for ch in range(3)]
            ch = ext.index(max(ext))                                               # first maximum: lower channel
            score = float(sum(c for _, c, _ in box)) * ext[ch]
            if best is None or score > best_score:                                 # strict: lower box index wins a tie
                best, best_score, best_ch = b, score, ch
        box = sorted(boxes[best], key=lambda e: (mean[e[0]][best_ch], e[0]))
        total, cum, cut = sum(c for _, c, _ in box), 0, None
        for j, (_, c, _) in enumerate(box):
            cum += c
            if 2 * cum >= total:
                cut = j
                break
        cut = min(cut, len(box) - 2)
        boxes[best] = box[:cut + 1]
        boxes.append(box[cut + 1:])
    for b, box in enumerate(boxes):
        c = sum(e[1] for e in box)
        pal[b] = [int(np.floor(sum(e[2][ch] for e in box) / c + 0.5)) for ch in range(3)]
    return pal, colors


def palette_map(pixels, palette):
    """Index of the nearest palette entry per pixel (squared RGB distance in integers), the smallest among equals."""
    p = np.asarray(pixels, dtype=np.uint8)
    flat = p.reshape(-1, 3).astype(np.int64)
    pal = np.asarray(palette, dtype=np.uint8).astype(np.int64)
    out = np.empty(flat.shape[0], dtype=np.uint8)
    for s in range(0, flat.shape[0], 4096):
        d = ((flat[s:s + 4096, None, :] - pal[None, :, :]) ** 2).sum(axis=2)
        out[s:s + 4096] = np.argmin(d, axis=1)                                     # argmin: the first minimum
    return out.reshape(p.shape[:-1])


def quantize(frames, mode="global"):
    """(palettes, n_used, indices) as inference.quantize_frames defines them."""
    frames = [np.asarray(f, dtype=np.uint8) for f in frames]
    if mode == "global":
        h = None
        for f in frames:
            h = color_histogram(f, h)
        pal, n = median_cut(h)
        return [pal], [n], [palette_map(f, pal[:n]) for f in frames]
    pals, ns, idx = [], [], []
    for f in frames:
        pal, n = median_cut(color_histogram(f))
        pals.append(pal)
        ns.append(n)
        idx.append(palette_map(f, pal[:n]))
    return pals, ns, idx


def depth_range(depth):
    x = np.nan_to_num(np.asarray(depth, dtype=np.float32))
    return np.float32(x.min()), np.float32(x.max())


def depth_colormap(depth, lut):
    """visualize_depth's array in float32, every operation rounded on its own; a NaN quotient gives index 0."""
    f32 = np.float32
    x = np.nan_to_num(np.asarray(depth, dtype=f32))
    mi, ma = f32(x.min()), f32(x.max())
    with np.errstate(over="ignore", invalid="ignore"):
        den = f32(f32(ma - mi) + f32(1e-8))
        q = ((x - mi).astype(f32) / den).astype(f32)
        y = (f32(255) * q).astype(f32)
    k = np.where(np.isnan(y), f32(0), y).astype(np.uint8)
    return np.asarray(lut, dtype=np.uint8)[k]


# ------------------------------------------------------------------------------------------------------------------
# LZW, minimum code size 8
# ------------------------------------------------------------------------------------------------------------------
def lzw_codes(indices):
    """The (code, width) sequence of GIF's LZW for a byte stream: clear first, clear again when 4096 codes are used."""
    data = bytes(bytearray(np.asarray(indices, dtype=np.uint8).reshape(-1).tolist()))
    codes = [(256, 9)]
    table = {bytes([i]): i for i in range(256)}
    nxt, width = 258, 9
    s = b""
    for i in range(len(data)):
        t = s + data[i:i + 1]
        if t in table:
            s = t
            continue
        codes.append((table[s], width))
        if nxt == (1 << width) and width < 12:
            width += 1
        if nxt < 4096:
            table[t] = nxt
            nxt += 1
        else:
            codes.append((256, width))
            table = {bytes([j]): j for j in range(256)}
            nxt, width = 258, 9
        s = data[i:i + 1]
    if s:
        codes.append((table[s], width))
        if nxt == (1 << width) and width < 12:
            width += 1
    codes.append((257, width))
    return codes


def lzw_encode(indices):
    acc = bits = 0
    out = bytearray()
    for code, width in lzw_codes(indices):
        acc |= code << bits
        bits += width
        while bits >= 8:
            out.append(acc & 255)
            acc >>= 8
            bits -= 8
    if bits:
        out.append(acc & 255)
    return bytes(out)


def lzw_decode(data):
    """(indices as bytes, number of clear codes read).  Raises ValueError on a malformed stream, including bytes left
    over after the end code beyond the padding of the last byte."""
    out = bytearray()
    acc = bits = pos = clears = 0
    width, table, prev = 9, None, None
    while True:
        while bits < width:
            if pos >= len(data):
                raise ValueError("no end code")
            acc |= data[pos] << bits
            pos += 1
            bits += 8
        code, acc, bits = acc & ((1 << width) - 1), acc >> width, bits - width
        if code == 256:
            table, prev, width = {i: bytes([i]) for i in range(256)}, None, 9
            nxt = 258
            clears += 1
            continue
        if code == 257:
            if pos != len(data) or acc != 0:
                raise ValueError("bytes after the end code")
            return bytes(out), clears
        if table is None:
            raise ValueError("no clear code first")
        if prev is None:
            entry = table[code]
        else:
            if code in table:
                entry = table[code]
            elif code == nxt and nxt < 4096:
                entry = prev + prev[:1]
            else:
                raise ValueError("code outside the table")
            if nxt < 4096:
                table[nxt] = prev + entry[:1]
                nxt += 1
        if nxt == (1 << width) and width < 12:
            width += 1
        out += entry
        prev = entry


# ------------------------------------------------------------------------------------------------------------------
# frames for the comparison with Pillow: smooth gradients plus noise, with and without a flat white surround
# ------------------------------------------------------------------------------------------------------------------
def synthetic_frame(h=96, w=128, surround=False, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([255 * x / (w - 1), 255 * y / (h - 1), 255 * (0.5 + 0.5 * np.sin(x / 17.0 + y / 11.0))], axis=2)
    img = np.clip(img + rng.normal(0.0, 6.0, img.shape), 0, 255)
    if surround:
        inside = ((y - h / 2) / (0.35 * h)) ** 2 + ((x - w / 2) / (0.35 * w)) ** 2 <= 1.0
        img[~inside] = 255.0
    return img.astype(np.uint8)


def mse(a, b):
    return float(((np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) ** 2).mean())
