"""CPU restatement of csrc/augment.hip in numpy -- test infrastructure only, like oracle/dzi_ref.py.

Parity with cv2 is UNPINNED: OpenCV is not installed and the reference holds no warped fixture, so the 8-bit warpAffine,
cvtColor (BGR<->HSV, BGR2GRAY) and blur arithmetic below is restated from OpenCV's documented fixed-point scheme and
held to known answers (tests/test_augment_host.py).  What IS pinned against the imported reference
(tests/golden/augment.npz, make_golden_augment.py): RandomOcclusion's rectangles and mask given the draws,
remove_invalids and generate_shiftscalerotate_matrix.  The GPU tests hold the kernels bit-equal to these functions.
"""
import math

import numpy as np

AB_BITS, INTER_BITS = 10, 5
AB_SCALE, INTER_TAB = 1 << AB_BITS, 1 << INTER_BITS
MAX_GT = 4
_M64 = 0xFFFFFFFFFFFFFFFF


# ---- warpAffine, 8-bit INTER_LINEAR (border 128) + INTER_NEAREST float mask (border 0) ---------------------------------
def inverse_affine(M):
    M = np.asarray(M, np.float64).reshape(2, 3)
    D = M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]
    D = 1.0 / D if D != 0.0 else 0.0
    m00, m01, m10, m11 = M[1, 1] * D, M[0, 1] * -D, M[1, 0] * -D, M[0, 0] * D
    b1 = -m00 * M[0, 2] - m01 * M[1, 2]
    b2 = -m10 * M[0, 2] - m11 * M[1, 2]
    return m00, m01, m10, m11, b1, b2


def _coords(M, Ho, Wo):
    m00, m01, m10, m11, b1, b2 = inverse_affine(M)
    x = np.arange(Wo, dtype=np.float64)
    y = np.arange(Ho, dtype=np.float64)
    ad = np.rint(m00 * x * AB_SCALE).astype(np.int64)[None, :]
    bd = np.rint(m10 * x * AB_SCALE).astype(np.int64)[None, :]
    X0 = np.rint((m01 * y + b1) * AB_SCALE).astype(np.int64)[:, None]
    Y0 = np.rint((m11 * y + b2) * AB_SCALE).astype(np.int64)[:, None]
    return X0 + ad, Y0 + bd


def tap_weights(fx, fy):
    """initInterTab2D's 15-bit bilinear weights: exact products * 32768, entry (0,0) = {32767, 0, 0, 1}."""
    w = [(INTER_TAB - fy) * (INTER_TAB - fx) * 32, (INTER_TAB - fy) * fx * 32, fy * (INTER_TAB - fx) * 32, fy * fx * 32]
    w = [np.asarray(v, np.int64).copy() for v in w]
    z = (fx == 0) & (fy == 0)
    w[0][z] = 32767
    w[3][z] = 1
    return w


def warp_u8(src, M, out_hw):
    """src (H,W,3) uint8, M forward (2,3) -> (Ho,Wo,3) uint8."""
    H, W, _ = src.shape
    Ho, Wo = out_hw
    Xa, Ya = _coords(M, Ho, Wo)
    rd = AB_SCALE // INTER_TAB // 2
    X = (Xa + rd) >> (AB_BITS - INTER_BITS)
    Y = (Ya + rd) >> (AB_BITS - INTER_BITS)
    sx, sy = X >> INTER_BITS, Y >> INTER_BITS
    fx, fy = X & (INTER_TAB - 1), Y & (INTER_TAB - 1)
    w = tap_weights(fx, fy)
    acc = np.zeros((Ho, Wo, 3), np.int64)
    for k in range(4):
        yy, xx = sy + (k >> 1), sx + (k & 1)
        ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        px = np.full((Ho, Wo, 3), 128, np.int64)
        px[ok] = src[yy[ok], xx[ok]]
        acc += px * w[k][:, :, None]
    return np.clip((acc + (1 << 14)) >> 15, 0, 255).astype(np.uint8)


def warp_mask(mask, M, out_hw):
    H, W = mask.shape
    Ho, Wo = out_hw
    Xa, Ya = _coords(M, Ho, Wo)
    X, Y = (Xa + AB_SCALE // 2) >> AB_BITS, (Ya + AB_SCALE // 2) >> AB_BITS
    ok = (X >= 0) & (X < W) & (Y >= 0) & (Y < H)
    out = np.zeros((Ho, Wo), np.float32)
    out[ok] = mask[Y[ok], X[ok]]
    return out


# ---- counter-based hash (occlusion bytes) --------------------------------------------------------------------------
def splitmix64(z):
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def pixel_hash(key, tag, b, pix, draw):
    ctr = (np.uint64(tag) << np.uint64(60)) ^ (np.uint64(draw) << np.uint64(56)) ^ (np.uint64(b) << np.uint64(36)) ^ \
        np.asarray(pix, np.uint64)
    return splitmix64(np.uint64(key & _M64) ^ splitmix64(ctr))


# ---- mask statistics / RandomOcclusion / remove_invalids ------------------------------------------------------------
def mask_stats(mask, max_id):
    """(max_id, 5) int {area, xmin, ymin, xmax, ymax} of mask == id, zeros when absent (to_visible_boxlist)."""
    out = np.zeros((max_id, 5), np.int64)
    for i in range(max_id):
        ys, xs = np.nonzero(mask == i + 1)
        if len(xs):
            out[i] = [len(xs), xs.min(), ys.min(), xs.max(), ys.max()]
    return out


def occlusion_rect(st, u, prob, H, W):
    """transform.py:257-290 with random.uniform(a, b) = a + (b - a) * u -> (x0, y0, x1, y1) or None."""
    x1, y1, x2, y2 = [int(float(v)) for v in st[1:5]]
    bw, bh = int(x2 - x1), int(y2 - y1)
    if not (0 + (1 - 0) * u[0] <= prob and bw > 2 and bh > 2):
        return None
    bb_size = bw * bh
    size = (0.02 + (0.7 - 0.02) * u[1]) * bb_size
    ratio = 0.5 + (2.0 - 0.5) * u[2]
    ew = int(np.sqrt(size * ratio))
    eh = int(np.sqrt(size / ratio))
    ecx = x1 + (x2 - x1) * u[3]
    ecy = y1 + (y2 - y1) * u[4]
    esx = int(np.clip((ecx - ew / 2 + 0.5), 0, W - 1))
    esy = int(np.clip((ecy - eh / 2 + 0.5), 0, H - 1))
    eex = int(np.clip((ecx + ew / 2 + 0.5), 0, W - 1))
    eey = int(np.clip((ecy + eh / 2 + 0.5), 0, H - 1))
    return esx, esy, eex, eey


def occlude(img, mask, n_inst, uniforms, prob, key, b):
    """In place on copies; -> (img, mask).  Boxes are taken once, before the loop (to_visible_boxlist)."""
    img, mask = img.copy(), mask.copy()
    H, W, _ = img.shape
    st = mask_stats(mask, max(MAX_GT, n_inst))
    for i in range(min(n_inst, MAX_GT)):
        r = occlusion_rect(st[i], uniforms[i], prob, H, W)
        if r is None:
            continue
        x0, y0, x1, y1 = r
        if x0 >= x1 or y0 >= y1:
            continue
        yy, xx = np.mgrid[y0:y1, x0:x1]
        h = pixel_hash(key, 1, b, (yy * W + xx).astype(np.uint64), 0)
        for c in range(3):
            img[y0:y1, x0:x1, c] = ((h >> np.uint64(8 * c)) & np.uint64(255)).astype(np.uint8)
        mask[y0:y1, x0:x1] = -1
    return img, mask


def relabel_lut(mask, n_inst, min_area=10):
    """remove_invalids: -> (kept instance indices, lut (n_inst + 1,)) -- id i+1 -> rank among kept, else 0."""
    keep, lut = [], np.zeros(n_inst + 1, np.float32)
    for i in range(n_inst):
        if (mask == i + 1).sum() >= min_area:
            keep.append(i)
            lut[i + 1] = len(keep)
    return keep, lut


def relabel(mask, lut):
    out = np.zeros_like(mask)
    for i in range(1, len(lut)):
        out[mask == i] = lut[i]
    return out


# ---- RandomHSV ------------------------------------------------------------------------------------------------------
def bgr2hsv_u8(img):
    """cv2.cvtColor(BGR2HSV) 8-bit: RGB2HSV_b, hsv_shift 12, hue range 180."""
    b, g, r = [img[:, :, c].astype(np.int64) for c in range(3)]
    v = np.maximum(np.maximum(b, g), r)
    vmin = np.minimum(np.minimum(b, g), r)
    diff = v - vmin
    vr = np.where(v == r, -1, 0)
    vg = np.where(v == g, -1, 0)
    with np.errstate(divide="ignore"):
        sdiv = np.where(v > 0, np.rint((255 << 12) / np.maximum(v, 1).astype(np.float64)), 0).astype(np.int64)
        hdiv = np.where(diff > 0, np.rint((180 << 12) / (6.0 * np.maximum(diff, 1))), 0).astype(np.int64)
    s = (diff * sdiv + (1 << 11)) >> 12
    h = (vr & (g - b)) + (~vr & ((vg & (b - r + 2 * diff)) + ((~vg) & (r - g + 4 * diff))))
    h = (h * hdiv + (1 << 11)) >> 12
    h = h + np.where(h < 0, 180, 0)
    return h, s, v


def hsv2bgr_u8(h, s, v):
    """cv2.cvtColor(HSV2BGR) 8-bit: float path on (h, s/255, v/255), cvRound(x * 255)."""
    f32 = np.float32
    hh = h.astype(f32)
    ss = s.astype(f32) * f32(1.0 / 255.0)
    vv = v.astype(f32) * f32(1.0 / 255.0)
    hh = hh * (f32(6.0) / f32(180.0))
    hh = np.where(hh < 0, hh + f32(6), np.where(hh >= 6, hh - f32(6), hh)).astype(f32)
    sector = np.floor(hh).astype(np.int64)
    hh = (hh - sector.astype(f32)).astype(f32)
    bad = (sector < 0) | (sector >= 6)
    sector[bad] = 0
    hh[bad] = 0
    one = f32(1.0)
    tab = np.stack([vv, vv * (one - ss), vv * (one - ss * hh), vv * (one - ss * (one - hh))]).astype(f32)
    sd = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])
    out = np.empty(h.shape + (3,), np.uint8)
    grey = ss == 0
    for c in range(3):
        val = np.take_along_axis(tab, sd[sector, c][None], 0)[0]
        val = np.where(grey, vv, val).astype(f32)
        out[:, :, c] = np.clip(np.rint(val * f32(255.0)), 0, 255).astype(np.uint8)
    return out


def distort_hsv(img, factors):
    """utils.py:181-195 given the three factors (float32): scale, clip at 179 / 255 when the factor is >= 1,
    truncating uint8 store."""
    h, s, v = bgr2hsv_u8(img)
    out = []
    for ch, f, lim in ((h, factors[0], 179), (s, factors[1], 255), (v, factors[2], 255)):
        x = ch.astype(np.float32) * np.float32(f)
        if not (np.float32(f) < 1):
            x = np.minimum(x, np.float32(lim))
        out.append(x.astype(np.int64))
    return hsv2bgr_u8(*out)


# ---- RandomSmooth / Grayscalize -------------------------------------------------------------------------------------
def box_blur(img, ks):
    """cv2.blur((ks, ks)), BORDER_REFLECT_101, cvRound(sum / ks^2)."""
    if ks <= 1:
        return img.copy()
    r = ks // 2
    H, W, _ = img.shape
    p = np.pad(img.astype(np.int64), ((r, r), (r, r), (0, 0)), mode="reflect")
    acc = np.zeros((H, W, 3), np.int64)
    for dy in range(ks):
        for dx in range(ks):
            acc += p[dy:dy + H, dx:dx + W]
    a = ks * ks
    return ((acc + a // 2) // a).astype(np.uint8)


def gray(img):
    """cv2 BGR2GRAY 8-bit fixed point, copied into 3 channels."""
    b, g, r = [img[:, :, c].astype(np.int64) for c in range(3)]
    y = ((1868 * b + 9617 * g + 4899 * r + 8192) >> 14).astype(np.uint8)
    return np.repeat(y[:, :, None], 3, axis=2)


def rotation_matrix_2d(center, angle, scale):
    """cv2.getRotationMatrix2D from its documented formula."""
    a = np.deg2rad(angle)
    alpha, beta = np.cos(a) * scale, np.sin(a) * scale
    cx, cy = center
    return np.array([[alpha, beta, (1 - alpha) * cx - beta * cy], [-beta, alpha, beta * cx + (1 - alpha) * cy]])


class Recorded:
    """Stands in for the `random` module with a list of u in [0,1): random() -> u, uniform(a, b) -> a + (b - a) u
    (random.uniform's formula), randint(a, b) -> a + int(u (b - a + 1))."""

    def __init__(self, us):
        self.us, self.i = list(us), 0

    def random(self):
        u = float(self.us[self.i])
        self.i += 1
        return u

    def uniform(self, a, b):
        return a + (b - a) * self.random()

    def randint(self, a, b):
        return a + int(self.random() * (b - a + 1))
