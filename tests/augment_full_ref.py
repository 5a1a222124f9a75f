"""CPU restatement in numpy of the two stages `--aug_chain full` adds to csrc/augment.hip (kd6d_aug_background,
kd6d_aug_sharpen) -- test infrastructure only, next to tests/augment_ref.py, whose box blur it imports.

Parity with cv2 is UNPINNED, as for warp / HSV / blur: OpenCV is not installed, so cv2.resize (8-bit INTER_LINEAR) and
cv2.normalize (NORM_MINMAX) are restated from OpenCV's documented arithmetic and held to closed-form answers
(tests/test_augment_full_host.py); the GPU tests hold the kernels bit-equal to these functions.  One known cv2 detail is
written down, not chased: for an exact 2x downscale cv2 switches INTER_LINEAR to its area path; this restatement (and
the kernel) stays bilinear at every scale.

cv2.resize, 8-bit INTER_LINEAR, per axis (d = output index, n = source extent, N = output extent):
    f  = float32((d + 0.5) * (double(n) / double(N)) - 0.5)          double arithmetic, rounded once to float32
    s  = floor(f);  f = f - float32(s)                               float32
    s < 0 -> s = 0, f = 0;      s >= n - 1 -> s = n - 1, f = 0;      taps s and min(s + 1, n - 1)
    c0 = rint((1 - f) * 2048),  c1 = rint(f * 2048)                  float32, ties to even: 11-bit coefficients
horizontal pass per source row:  h = p[x0] * a0 + p[x1] * a1         int, scaled by 2^11
vertical pass:                   out = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2
"""
import numpy as np

from augment_ref import box_blur

RESIZE_COEF_SCALE = 2048
DBL_EPSILON = float(np.finfo(np.float64).eps)


def resize_taps(n_dst, n_src):
    """-> (i0, i1, c0, c1), each (n_dst,) int64: the two taps of every output index and their 11-bit coefficients."""
    f32 = np.float32
    d = np.arange(n_dst, dtype=np.float64)
    f = ((d + 0.5) * (float(n_src) / float(n_dst)) - 0.5).astype(f32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(f32)).astype(f32)
    lo, hi = s < 0, s >= n_src - 1
    s = np.where(lo, 0, np.where(hi, n_src - 1, s))
    f = np.where(lo | hi, f32(0), f).astype(f32)
    c0 = np.rint((f32(1) - f) * f32(RESIZE_COEF_SCALE)).astype(np.int64)
    c1 = np.rint(f * f32(RESIZE_COEF_SCALE)).astype(np.int64)
    return s, np.minimum(s + 1, n_src - 1), c0, c1


def resize_u8(img, out_hw):
    """cv2.resize(img, (W, H)) for (h, w, 3) uint8, 8-bit INTER_LINEAR -> (H, W, 3) uint8."""
    H, W = out_hw
    h, w, _ = img.shape
    x0, x1, a0, a1 = resize_taps(W, w)
    y0, y1, b0, b1 = resize_taps(H, h)
    src = img.astype(np.int64)
    rows = src[:, x0] * a0[None, :, None] + src[:, x1] * a1[None, :, None]            # (h, W, 3), scaled by 2^11
    h0, h1 = rows[y0], rows[y1]
    out = (((b0[:, None, None] * (h0 >> 4)) >> 16) + ((b1[:, None, None] * (h1 >> 4)) >> 16) + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def merge_background(frame, mask, back):
    """transform.py:182-190 merge_background_mask: mask == 0 pixels take cv2.resize(back, frame size), the others
    (instance ids, the occlusion's -1) keep the frame's byte."""
    H, W, _ = frame.shape
    if back.shape != frame.shape:
        back = resize_u8(back, (H, W))
    out = frame.copy()
    z = mask == 0
    out[z] = back[z]
    return out


def normalize_minmax_params(mn, mx):
    """cv2.normalize(NORM_MINMAX, alpha=0, beta=255): (scale, shift) in double."""
    mn, mx = float(mn), float(mx)
    scale = 255.0 * (1.0 / (mx - mn) if mx - mn > DBL_EPSILON else 0.0)
    return scale, 0.0 - mn * scale


def _trunc_u8(x):
    i = x.astype(np.int64)                   # truncation toward zero, as numpy's float -> uint8 cast of in-range values
    assert i.min() >= 0 and i.max() <= 255
    return i.astype(np.uint8)


def pencil_sharpen(img, ks, ratio_mode, alpha, return_pre=False):
    """transform.py:115-128 RandomPencilSharpen.__call__ past its coin, with the reference's dtypes.  ks = 0: a copy.
    return_pre: also the two pre-truncation images (float32 edge after scale-and-shift, float64 blend after it)."""
    if ks == 0:
        return img.copy()
    f32 = np.float32
    s = box_blur(img, ks)
    if ratio_mode:
        edge = img.astype(f32) / (s.astype(f32) + f32(0.01))
    else:
        edge = img.astype(f32) - s.astype(f32)
    edge = edge.astype(f32)
    scale, shift = normalize_minmax_params(edge.min(), edge.max())
    pre_e = (edge * f32(scale)).astype(f32) + f32(shift)
    e = _trunc_u8(pre_e)
    alpha = float(alpha)
    v = img.astype(np.float64) * (1.0 - alpha) + e.astype(np.float64) * alpha
    scale, shift = normalize_minmax_params(v.min(), v.max())
    pre_o = v * scale + shift
    out = _trunc_u8(pre_o)
    return (out, pre_e, pre_o) if return_pre else out
