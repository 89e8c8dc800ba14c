"""Output image: film -> 8-bit sRGB -> PNG (the headless half of src/main.cpp).

``film_to_image`` is the C-ABI ``vpt_film_to_srgb8`` (film_to_image, src/main.cpp:12-24, with the
xyz_to_linsrgb / linsrgb_to_srgb of include/vpt/color.hpp:8-30).  ``save_png`` writes what
``Image<unsigned char,3>::save`` writes (src/image_io.cpp:18-58: 8-bit truecolor, no alpha, rows
top to bottom); the pixel bytes are identical, the deflate stream is zlib's rather than spng's.
"""
from __future__ import annotations

import ctypes as C
import struct
import zlib
from pathlib import Path

import numpy as np

from . import capi


def film_to_image(film: np.ndarray) -> np.ndarray:
    """float32 [H][W][4] XYZW film -> uint8 [H][W][3] sRGB image."""
    film = np.ascontiguousarray(film, dtype=np.float32)
    if film.ndim != 3 or film.shape[2] != 4:
        raise ValueError(f"film must be [H][W][4], got {film.shape}")
    h, w = film.shape[:2]
    out = np.empty((h, w, 3), dtype=np.uint8)
    L = capi.lib()
    capi.check(L.vpt_film_to_srgb8(film.ctypes.data_as(C.POINTER(C.c_float)), w, h,
                                   out.ctypes.data_as(C.POINTER(C.c_uint8))), "vpt_film_to_srgb8")
    return out


def foreground_film(film: np.ndarray, alpha: np.ndarray, cfg) -> np.ndarray:
    """The film of the medium alone: removes the environment light seen through it.  A path that leaves the volume
    unhit carries exactly the environment light (plus emission picked up at null collisions), so with the matte
    `alpha` (Integrator.render_alpha) the film is w * imaging_ratio * ((1 - alpha) * Le + alpha * C) and

        xyz' = max(film.xyz - (1 - alpha) * w * imaging_ratio * infinite_light_xyz * multiplier, 0) / alpha

    where alpha > 1/255 (a matte that rounds to at least one 8-bit step), else 0; w is kept.  float32 throughout.
    The result goes through film_to_image as any film; pair it with the alpha plane as straight alpha."""
    film = np.asarray(film, dtype=np.float32)
    alpha = np.asarray(alpha, dtype=np.float32)
    if film.ndim != 3 or film.shape[2] != 4 or alpha.shape != film.shape[:2]:
        raise ValueError(f"foreground_film wants film [H][W][4] and alpha [H][W], got {film.shape} and {alpha.shape}")
    wp = cfg.worker_parameters
    le = np.asarray(wp.infinite_light_xyz[:], np.float32) * np.float32(wp.infinite_light_multiplier)
    r = np.float32(cfg.camera_parameters.imaging_ratio)
    env = ((np.float32(1) - alpha) * film[..., 3] * r)[..., None] * le
    out = film.copy()
    cover = alpha > np.float32(1.0 / 255.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        fg = np.maximum(film[..., :3] - env, np.float32(0)) / alpha[..., None]
    out[..., :3] = np.where(cover[..., None], fg, np.float32(0))
    return out


def relight(groups: np.ndarray, gains) -> np.ndarray:
    """The relit film of light-group planes (Integrator.set_light_groups; float32 [3][H][W][4]: emission, sun, sky)
    under `gains` (3 x 3, [group][XYZ]; scenes.light_gains): per pixel

        out.c = ((G0.c * k0.c) + (G1.c * k1.c)) + (G2.c * k2.c)   for c = X, Y, Z;     out.w = G0.w

    in float32, in this order -- vpt_gpu_relight's arithmetic restated in numpy, byte for byte, so a machine without a
    device relights a saved file (--groups-out / --relight-from)."""
    g = np.asarray(groups, dtype=np.float32)
    k = np.asarray(gains, dtype=np.float32).reshape(-1)
    if g.ndim != 4 or g.shape[0] != 3 or g.shape[3] != 4 or k.size != 9:
        raise ValueError(f"relight wants planes [3][H][W][4] and 3 x 3 gains, got {g.shape} and {k.size} gains")
    k = k.reshape(3, 3)
    out = np.empty(g.shape[1:], np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        out[..., :3] = ((g[0, ..., :3] * k[0]) + (g[1, ..., :3] * k[1])) + (g[2, ..., :3] * k[2])
    out[..., 3] = g[0, ..., 3]
    return out


def _chunk(tag: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def encode_png(rgb: np.ndarray) -> bytes:
    """uint8 [H][W][3] (or uint16) -> PNG bytes (truecolor, filter 0 per row); [H][W][4] -> truecolor with
    (straight) alpha, colour type 6."""
    rgb = np.ascontiguousarray(rgb)
    if rgb.ndim != 3 or rgb.shape[2] not in (3, 4) or rgb.dtype not in (np.uint8, np.uint16):
        raise ValueError("encode_png wants uint8/uint16 [H][W][3] or [H][W][4]")
    h, w = rgb.shape[:2]
    depth = 8 * rgb.dtype.itemsize
    rows = rgb.astype(rgb.dtype.newbyteorder(">"), copy=False).reshape(h, -1).view(np.uint8)
    raw = np.concatenate([np.zeros((h, 1), np.uint8), rows], axis=1).tobytes()
    ihdr = struct.pack(">IIBBBBB", w, h, depth, 2 if rgb.shape[2] == 3 else 6, 0, 0, 0)
    return (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(raw, 6))
            + _chunk(b"IEND", b""))


def save_png(path, rgb: np.ndarray) -> None:
    Path(path).write_bytes(encode_png(rgb))


def decode_png(data: bytes) -> np.ndarray:
    """Minimal reader for truecolor 8/16-bit non-interlaced PNGs, with or without alpha (tests and tools):
    [H][W][3] for colour type 2, [H][W][4] for colour type 6."""
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError("not a PNG")
    pos, idat, hdr = 8, [], None
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if tag == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat.append(body)
        pos += 12 + n
    w, h, depth, ctype, _, _, interlace = hdr
    if ctype not in (2, 6) or interlace != 0 or depth not in (8, 16):
        raise ValueError("decode_png supports truecolor 8/16-bit non-interlaced only")
    ch = 3 if ctype == 2 else 4
    bpp = ch * depth // 8
    raw = np.frombuffer(zlib.decompress(b"".join(idat)), np.uint8).reshape(h, 1 + w * bpp)
    if not raw[:, 0].any():  # every row unfiltered (what encode_png writes)
        out = raw[:, 1:].astype(np.int32)
    else:
        out = _unfilter(raw, h, w * bpp, bpp)
    img = out.astype(np.uint8)
    if depth == 16:
        return img.reshape(h, w * ch, 2).view(">u2").reshape(h, w, ch).astype(np.uint16)
    return img.reshape(h, w, ch)


def _unfilter(raw, h, stride, bpp):
    out = np.zeros((h, stride), np.int32)
    prev = np.zeros(stride, np.int32)
    for y in range(h):
        f, line = raw[y, 0], raw[y, 1:].astype(np.int32)
        cur = np.zeros_like(line)
        for x in range(stride):
            a = cur[x - bpp] if x >= bpp else 0
            b, c = prev[x], (prev[x - bpp] if x >= bpp else 0)
            if f == 0:
                p = 0
            elif f == 1:
                p = a
            elif f == 2:
                p = b
            elif f == 3:
                p = (a + b) // 2
            else:
                pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                p = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
            cur[x] = (line[x] + p) & 0xFF
        out[y], prev = cur, cur
    return out
