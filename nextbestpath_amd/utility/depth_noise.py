"""The depth-sensor noise model: the DEFINITION (numpy, CPU) that csrc/nbp_depth_noise.hip equals bit for bit.
Not in the reference, whose imperfect-depth mode is a learned depth network that is outside this build.

A frame's noise depends on (word seed, frame id, pixel) only, through counter-based 32-bit words:
    mix(x):     x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16          (uint32, wrapping)
    key       = mix(mix(seed ^ 0x9E3779B9) + frame)
    word(p,k) = mix(mix((8 p + k) ^ key) + key),  p = row W + col,  k = 0..4                          (H W <= 2^29)
Gaussian stand-in: s = the sum of the 16 bytes of word(p, 0..3) (an Irwin-Hall sum: mean 2040, variance 16 (256^2 - 1) / 12),
g = (float32(s) - 2040) * float32(1 / sqrt(16 (256^2 - 1) / 12)): 4081 levels, |g| <= 6.9.  This is a deliberate choice over
Box-Muller: no log / cos, whose device and host implementations round differently -- integer arithmetic and two exact fp32
operations are the same bits on both sides, so the kernel can be pinned against this file exactly.
Axial noise, five fp32 operations in this order, no contraction:
    t = z z;  s = sigma_quad t;  s = sigma_base + s;  d = s g;  zn = z + d;  zn = max(zn, z_min)
Dropout: the pixel is dropped iff word(p, 4) < thr, thr = min(2^32 - 1, floor(dropout 2^32)) (formed on the host in double).
Edge (flying-pixel) dropout, edge_threshold > 0: a valid pixel is dropped iff some 4-neighbour inside the image is valid and
|z - z_nb| > edge_threshold, in fp32 on the CLEAN depths; neighbours outside the image and background neighbours do not count.
Output: zn where the clean pixel is valid (z > -1) and not dropped, -1 otherwise.
"""
from __future__ import annotations

import math
import numbers

import numpy as np

f32, u32 = np.float32, np.uint32

G_MEAN = f32(2040.0)
G_SCALE = f32(0.0033829375)             # fp32(1 / sqrt(16 (256^2 - 1) / 12))
MAX_PIXELS = 1 << 29
CAMERA_SEED_STRIDE = 7919               # a camera's word seed = (spec seed + 7919 camera seed) mod 2^32

_DEFAULTS = {"sigma_base": 0.0, "sigma_quad": 0.0, "dropout": 0.0, "edge_threshold": 0.0, "z_min": 0.5, "seed": 0}


def option_spec(x):
    """The option `depth_noise` -> None (off) or the normalised spec: a dict with exactly the keys sigma_base, sigma_quad, dropout,
    edge_threshold (0 = off), z_min (floats) and seed (int).  None = off; a dict with any of those keys (edge_threshold may be None)
    fills the rest with the defaults 0, 0, 0, off, 0.5, 0.  ValueError on anything else: another type (there is no `True` preset:
    nobody has measured what a typical sensor is in these scene units), unknown keys, negative or non-finite values, dropout >= 1,
    z_min <= 0."""
    if x is None:
        return None
    if not isinstance(x, dict):
        raise ValueError("depth_noise: None or a dict with the keys " + " / ".join(_DEFAULTS) + " expected")
    unknown = sorted(set(x) - set(_DEFAULTS), key=str)
    if unknown:
        raise ValueError(f"depth_noise: unknown keys {unknown}")
    out = {}
    for k, default in _DEFAULTS.items():
        v = x.get(k, default)
        if k == "edge_threshold" and v is None:
            v = 0.0
        if k == "seed":
            if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 0:
                raise ValueError(f"depth_noise: seed must be a non-negative integer, got {v!r}")
            out[k] = int(v)
            continue
        if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v) or v < 0:
            raise ValueError(f"depth_noise: {k} must be a finite non-negative number, got {v!r}")
        out[k] = float(v)
    if out["dropout"] >= 1.0:
        raise ValueError(f"depth_noise: dropout must lie in [0, 1), got {out['dropout']}")
    if out["z_min"] <= 0.0:
        raise ValueError(f"depth_noise: z_min must be positive, got {out['z_min']}")
    return out


def dropout_threshold(dropout):
    """thr of the dropout test word(p, 4) < thr."""
    return min((1 << 32) - 1, int(math.floor(float(dropout) * 4294967296.0)))


def word_seed(spec, camera_seed):
    """The word seed of a camera: (spec seed + 7919 camera seed) mod 2^32."""
    return (int(spec["seed"]) + CAMERA_SEED_STRIDE * int(camera_seed)) % (1 << 32)


def mix(x):
    """The 32-bit finaliser, on a uint32 array (wrapping)."""
    x = np.array(x, dtype=u32, ndmin=1)
    x ^= x >> u32(16)
    x *= u32(0x7feb352d)
    x ^= x >> u32(15)
    x *= u32(0x846ca68b)
    x ^= x >> u32(16)
    return x


def frame_key(seed, frame):
    s = u32(int(seed) & 0xFFFFFFFF) ^ u32(0x9E3779B9)
    return int(mix(mix(s) + np.array([int(frame) & 0xFFFFFFFF], u32))[0])


def words(p, k, key):
    """word(p, k) for a uint32 array of pixel indices p."""
    key = u32(key)
    x = (np.asarray(p, u32) * u32(8) + u32(k)) ^ key
    return mix(mix(x) + key)


def gaussian(p, key):
    """g(p) for a uint32 array of pixel indices: fp32."""
    s = np.zeros(np.shape(p), u32)
    for k in range(4):
        w = words(p, k, key).reshape(np.shape(p))
        s += (w & u32(255)) + ((w >> u32(8)) & u32(255)) + ((w >> u32(16)) & u32(255)) + (w >> u32(24))
    return (s.astype(f32) - G_MEAN) * G_SCALE


def edge_mask(z, edge_threshold):
    """The flying-pixel test on clean depths z [H,W] fp32: True where a valid pixel has a valid 4-neighbour further than the threshold."""
    thr = f32(edge_threshold)
    valid = z > f32(-1.0)
    hit = np.zeros(z.shape, bool)

    def test(a, b, va, vb):                     # a and b are neighbours: both dropped when both valid and far apart
        return va & vb & (np.abs(a - b) > thr)
    h = test(z[:, 1:], z[:, :-1], valid[:, 1:], valid[:, :-1])
    hit[:, 1:] |= h
    hit[:, :-1] |= h
    v = test(z[1:, :], z[:-1, :], valid[1:, :], valid[:-1, :])
    hit[1:, :] |= v
    hit[:-1, :] |= v
    return hit


def apply(z_clean, seed, frame, spec):
    """z_clean [H,W] fp32, word seed, frame id, spec (option_spec's or its argument) -> the noisy frame [H,W] fp32."""
    spec = option_spec(spec)
    if spec is None:
        raise ValueError("depth_noise.apply needs a spec (None means off: there is nothing to apply)")
    z = np.ascontiguousarray(z_clean, f32)
    if z.ndim != 2 or z.size < 1 or z.size > MAX_PIXELS:
        raise ValueError(f"depth_noise.apply: one [H,W] frame of at most 2^29 pixels expected, got shape {z.shape}")
    H, W = z.shape
    key = frame_key(seed, frame)
    p = np.arange(H * W, dtype=u32).reshape(H, W)
    g = gaussian(p, key)
    t = z * z
    s = f32(spec["sigma_quad"]) * t
    s = f32(spec["sigma_base"]) + s
    d = s * g
    zn = z + d
    zn = np.maximum(zn, f32(spec["z_min"]))
    keep = z > f32(-1.0)
    thr = dropout_threshold(spec["dropout"])
    if thr > 0:
        keep &= ~(words(p, 4, key).reshape(H, W) < u32(thr))
    if spec["edge_threshold"] > 0:
        keep &= ~edge_mask(z, spec["edge_threshold"])
    return np.where(keep, zn, f32(-1.0)).astype(f32)
