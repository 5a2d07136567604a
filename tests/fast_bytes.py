"""numpy model of the byte form of the FAST kernel's pair test (csrc/orb_kernels.hip, fast_nms_kernel, phase 1) and the
test image that sits on its boundaries; shared by tests/test_fast_bytes_cpu.py and tests/test_gpu_fast_bytes.py.

The kernel keeps the four pixels of a dword group as four bytes of one register and asks, per ring pixel r and centre v,
"r >= v - thr" (not darker) and "r > v + thr" (brighter) with v_lerp_u8, which computes (a + b + (c & 1)) >> 1 per byte
on a 9-bit sum: bit 7 of the result is the carry of a + b + (c & 1).  With n = 255 - v (~v as a byte),
    Yd = min(n + thr, 255):  bit 7 of lerp(r, Yd, 1)  <=>  r + Yd >= 255  <=>  r >= v - thr
    Yb = max(n - thr, 0):    bit 7 of lerp(r, Yb, 0)  <=>  r + Yb >= 256  <=>  r >  v + thr
saturated ends included (Yd = 255: always, Yb = 0: never).  A darker arc is possible unless some opposite pair holds two
not-darker pixels; a brighter arc is possible when every opposite pair holds a brighter pixel."""
import numpy as np

from tests.fast_sides import CIRC, PAIRS


def thresholds(v, thr):
    """(Yd, Yb) of the centre bytes v"""
    n = 255 - np.asarray(v, np.int32)
    return np.minimum(n + thr, 255), np.maximum(n - thr, 0)


def lerp_u8(a, b, c):
    """one byte of v_lerp_u8: 9-bit sum, rounding bit from c"""
    return ((np.asarray(a, np.int32) + np.asarray(b, np.int32) + (c & 1)) >> 1) & 0xFF


def flags(v, r, thr):
    """bit 7 of the two lerps: (not darker, brighter), as booleans"""
    yd, yb = thresholds(v, thr)
    return (lerp_u8(r, yd, 1) & 0x80) != 0, (lerp_u8(r, yb, 0) & 0x80) != 0


def sides(v, r, thr):
    """phase 1's flags from the byte form: (darker arc possible, brighter arc possible); v [..], r [16, ..]"""
    nd, br = flags(v[None], r, thr)
    no_dark = np.zeros(v.shape, bool)
    brt = np.ones(v.shape, bool)
    for a, b in PAIRS:
        no_dark |= nd[a] & nd[b]
        brt &= br[a] | br[b]
    return ~no_dark, brt


def centres(thr):
    return [0, 1, thr - 1, thr, thr + 1, 128, 254 - thr, 255 - thr, 256 - thr, 254, 255]


def boundary_stamps(thr, W=640, H=480, seed=12):
    """9 x 9 stamps on a 9-pixel grid.  A stamp is flat at its centre value v (cycling through centres(thr)) but for its
    ring: an arc of 7-11 ring pixels at v -/+ thr or v -/+ (thr + 1) (one of the two for the whole arc in three stamps
    of four, a mix per pixel in the fourth), the rest of the ring at v -/+ {0, thr - 1, thr}; everything clipped to
    0..255.  The side (darker: minus, brighter: plus) is random per stamp."""
    rng = np.random.default_rng(seed + thr)
    img = np.full((H, W), 128, np.uint8)
    cs = centres(thr)
    i = 0
    for y in range(4, H - 4, 9):
        for x in range(4, W - 4, 9):
            v = cs[i % len(cs)]
            i += 1
            sign = -1 if rng.integers(2) else 1
            start, length, mode = rng.integers(16), rng.integers(7, 12), rng.integers(4)
            img[y - 4:y + 5, x - 4:x + 5] = v
            for k, (dx, dy) in enumerate(CIRC):
                if (k - start) % 16 < length:
                    d = thr + (1 if mode < 2 else 0 if mode == 2 else rng.integers(2))
                else:
                    d = (0, thr - 1, thr)[rng.integers(3)]
                img[y + dy, x + dx] = np.clip(v + sign * d, 0, 255)
    return img
