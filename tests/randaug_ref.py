"""CPU restatement of the reference's RandAugment (datasets/randaugment.py: RandAugment, augment_list, affine_transform)
in NumPy, byte for byte what Pillow computes for the 14 operations of augment_list.  tests/test_randaugment_cpu.py pins it
to live Pillow and to the fixture recorded from the reference (tests/golden/randaugment_golden.npz); it is the only
authority the kernels are compared with.

An image is uint8 [H, W, 3], a label map uint8 [H, W] or None; a program is a list of (op name, signed value) as
RandAugment.get_params draws it: the shear, the translation in PIXELS, the angle in degrees, the Solarize threshold
(float), the Posterize bits (int), the blend factor; 0.0 for the operations without a magnitude."""
import json
import math
import os

import numpy as np

import colorjit_ref as CR

OPS = ("Identity", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "AutoContrast", "Invert", "Equalize",
       "Solarize", "Posterize", "Color", "Brightness", "Sharpness")          # = SSA_RANDAUG_* of include/semseg_hip.h
RANGES = ((0., 1.0), (0., 0.3), (0., 0.3), (0., 0.33), (0., 0.33), (0, 30), (0, 1), (0, 1), (0, 1), (0, 110), (4, 8),
          (0.1, 1.9), (0.1, 1.9), (0.1, 1.9))                                # augment_list's (minval, maxval)
GEOMETRIC = ("ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate")
F64 = np.float64


# ------------------------------------------------------------------ the affine warps
def warp_bilinear(img, a, fill=0):
    """img.transform(size, AFFINE, a, BILINEAR, fillcolor): libImaging/Geometry.c affine_transform + bilinear_filter,
    all in double, left to right, the result truncated."""
    H, W = img.shape[:2]
    a0, a1, a2, a3, a4, a5 = (F64(v) for v in a)
    x = (np.arange(W, dtype=F64) + 0.5)[None, :]
    y = (np.arange(H, dtype=F64) + 0.5)[:, None]
    xin = a0 * x + a1 * y + a2
    yin = a3 * x + a4 * y + a5
    inside = (xin >= 0.0) & (xin < W) & (yin >= 0.0) & (yin < H)
    xs, ys = xin - 0.5, yin - 0.5
    xf, yf = np.floor(xs), np.floor(ys)
    dx, dy = (xs - xf)[..., None], (ys - yf)[..., None]
    xi, yi = np.where(inside, xf, 0).astype(np.int64), np.where(inside, yf, 0).astype(np.int64)
    x0, x1 = np.clip(xi, 0, W - 1), np.clip(xi + 1, 0, W - 1)
    yc = np.clip(yi, 0, H - 1)
    y1ok = ((yi + 1 >= 0) & (yi + 1 < H))[..., None]
    y1 = np.clip(yi + 1, 0, H - 1)
    p = img.reshape(H, W, -1).astype(F64)
    v1 = p[yc, x0] + (p[yc, x1] - p[yc, x0]) * dx
    v2 = np.where(y1ok, p[y1, x0] + (p[y1, x1] - p[y1, x0]) * dx, v1)
    v = v1 + (v2 - v1) * dy
    out = np.where(inside[..., None], v.astype(np.int64), fill).astype(np.uint8)
    return out.reshape(img.shape)


def fix16(v):
    """FIX(v) = FLOOR(v * 65536 + 0.5) of Geometry.c"""
    return int(math.floor(float(v) * 65536.0 + 0.5))


def fixed_coefficients(a):
    """The six 16.16 coefficients of affine_fixed: the half-pixel offset goes into a2 and a5 before fixing."""
    a0, a1, a2, a3, a4, a5 = (float(v) for v in a)
    return (fix16(a0), fix16(a1), fix16(a2 + a0 * 0.5 + a1 * 0.5), fix16(a3), fix16(a4), fix16(a5 + a3 * 0.5 + a4 * 0.5))


def warp_nearest_fixed(img, a, fill):
    """img.transform(size, AFFINE, a, NEAREST, fillcolor) for a matrix with a1 != 0 or a3 != 0: Pillow's 16.16 fixed-point
    path (affine_fixed).  An integer recurrence: the closed form below is the same value."""
    H, W = img.shape[:2]
    f0, f1, f2, f3, f4, f5 = fixed_coefficients(a)
    x = np.arange(W, dtype=np.int64)[None, :]
    y = np.arange(H, dtype=np.int64)[:, None]
    xin = (f2 + y * f1 + x * f0) >> 16
    yin = (f5 + y * f4 + x * f3) >> 16
    inside = (xin >= 0) & (xin < W) & (yin >= 0) & (yin < H)
    src = img[np.clip(yin, 0, H - 1), np.clip(xin, 0, W - 1)]
    return np.where(inside if img.ndim == 2 else inside[..., None], src, fill).astype(np.uint8)


def running_coordinates(start, n):
    """int64[n]: ImagingScaleAffine's source index of every output index at scale 1 -- a double that starts at `start`
    and grows by 1.0 per step, every sum rounded, truncated toward zero; -1 when negative (COORD)."""
    steps = np.full(n, 1.0, dtype=F64)
    steps[0] = F64(start)
    pos = np.cumsum(steps)                          # sequential, as the C loop adds
    return np.where(pos < 0.0, -1, np.trunc(pos)).astype(np.int64)


def warp_nearest_scale(img, a, fill):
    """img.transform(size, AFFINE, a, NEAREST, fillcolor) for a1 == a3 == 0 and a0 == a4 == 1 (the two translations):
    Pillow takes ImagingScaleAffine there, not the fixed-point path."""
    H, W = img.shape[:2]
    a0, a1, a2, a3, a4, a5 = (float(v) for v in a)
    assert a1 == 0 and a3 == 0 and a0 == 1 and a4 == 1
    xin = running_coordinates(a2 + a0 * 0.5, W)[None, :]
    yin = running_coordinates(a5 + a4 * 0.5, H)[:, None]
    inside = (xin >= 0) & (xin < W) & (yin >= 0) & (yin < H)
    src = img[np.clip(yin, 0, H - 1), np.clip(xin, 0, W - 1)]
    return np.where(inside if img.ndim == 2 else inside[..., None], src, fill).astype(np.uint8)


def warp_nearest(img, a, fill):
    return warp_nearest_scale(img, a, fill) if a[1] == 0 and a[3] == 0 else warp_nearest_fixed(img, a, fill)


def rotate_matrix(angle, w, h):
    """Image.rotate's matrix for angle % 360 != 0 (no centre, no translation, no expansion)."""
    angle = -math.radians(angle % 360.0)
    m = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0,
         round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]
    cx, cy = w / 2.0, h / 2.0
    x, y = -cx, -cy
    m[2], m[5] = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
    m[2] += cx
    m[5] += cy
    return m


def matrix_of(op, value, w, h):
    """The affine coefficients of a geometric operation (None: Rotate by a multiple of 360 degrees, a copy)."""
    v = float(value)
    if op == "ShearX":
        return [1, v, 0, 0, 1, 0]
    if op == "ShearY":
        return [1, 0, 0, v, 1, 0]
    if op == "TranslateX":
        return [1, 0, v, 0, 1, 0]
    if op == "TranslateY":
        return [1, 0, 0, 0, 1, v]
    assert op == "Rotate"
    return None if v % 360.0 == 0 else rotate_matrix(v, w, h)


# ------------------------------------------------------------------ the table operations
def histogram(img):
    return np.stack([np.bincount(img[..., c].ravel(), minlength=256) for c in range(3)]).astype(np.int64)


def autocontrast_lut(h):
    """ImageOps.autocontrast (cutoff 0) of one band's histogram."""
    nz = np.nonzero(h)[0]
    lo, hi = int(nz[0]), int(nz[-1])
    if hi <= lo:
        return np.arange(256)
    scale = 255.0 / (hi - lo)
    offset = -lo * scale
    return np.array([min(max(int(i * scale + offset), 0), 255) for i in range(256)])


def equalize_lut(h):
    """ImageOps.equalize of one band's histogram; entries above 255 are CLIPPED by Image.point, not wrapped."""
    nz = [int(v) for v in h if v]
    if len(nz) <= 1:
        return np.arange(256)
    step = (sum(nz) - nz[-1]) // 255
    if not step:
        return np.arange(256)
    lut, n = [], step // 2
    for i in range(256):
        lut.append(min(n // step, 255))
        n += int(h[i])
    return np.array(lut)


def _by_band(img, lut_of):
    h = histogram(img)
    return np.stack([lut_of(h[c])[img[..., c]] for c in range(3)], -1).astype(np.uint8)


def autocontrast(img):
    return _by_band(img, autocontrast_lut)


def equalize(img):
    return _by_band(img, equalize_lut)


def invert(img):
    return (255 - img.astype(np.int64)).astype(np.uint8)


def solarize(img, threshold):
    return np.where(img.astype(F64) < float(threshold), img, 255 - img.astype(np.int64)).astype(np.uint8)


def posterize(img, bits):
    return (img & np.uint8(~(2 ** (8 - int(bits)) - 1) & 255)).astype(np.uint8)


def smooth(img):
    """ImageFilter.SMOOTH: (1,1,1,1,5,1,1,1,1) / 13 + 0.5 truncated, the border rows and columns copied.  Pillow sums in
    float32; s / 13 + 0.5 is never closer than 1/26 to an integer (2 s + 13 is odd), so the integer form is the same byte."""
    out = img.copy()
    H, W = img.shape[:2]
    if H < 3 or W < 3:
        return out
    p = img.astype(np.int64)
    s = sum(p[dy:H - 2 + dy, dx:W - 2 + dx] for dy in range(3) for dx in range(3)) + 4 * p[1:-1, 1:-1]
    out[1:-1, 1:-1] = (2 * s + 13) // 26
    return out


def sharpness(img, v):
    return CR.blend(smooth(img), img, v)


# ------------------------------------------------------------------ one operation, a chain
def apply_op(img, lab, op, value, fill_label=255):
    """-> (img, lab) after one operation of augment_list with its signed value."""
    if op in GEOMETRIC:
        a = matrix_of(op, value, img.shape[1], img.shape[0])
        if a is None:
            return img, lab
        img = warp_nearest(img, a, 0) if op == "Rotate" else warp_bilinear(img, a, 0)
        return img, (None if lab is None else warp_nearest(lab, a, fill_label))
    if op == "AutoContrast":
        img = autocontrast(img)
    elif op == "Invert":
        img = invert(img)
    elif op == "Equalize":
        img = equalize(img)
    elif op == "Solarize":
        img = solarize(img, value)
    elif op == "Posterize":
        img = posterize(img, value)
    elif op == "Color":
        img = CR.saturation(img, value)
    elif op == "Brightness":
        img = CR.brightness(img, value)
    elif op == "Sharpness":
        img = sharpness(img, value)
    else:
        assert op == "Identity", op
    return img, lab


def augment(img, lab, program, window=None, flip=False, fill_label=255):
    """The program on the crop window (x0, y0, w, h) of the pair, mirrored first under `flip` (the reference crops and
    flips before RandAugment: datasets/__init__.py:83-87)."""
    if window is not None:
        x0, y0, w, h = window
        img = img[y0:y0 + h, x0:x0 + w]
        lab = None if lab is None else lab[y0:y0 + h, x0:x0 + w]
    if flip:
        img = img[:, ::-1]
        lab = None if lab is None else lab[:, ::-1]
    img = np.ascontiguousarray(img)
    lab = None if lab is None else np.ascontiguousarray(lab)
    for op, value in program:
        img, lab = apply_op(img, lab, op, value, fill_label)
    return img, lab


def magnitude(op, m):
    """val of RandAugment.__call__ for the operation at magnitude m, unsigned and before the size factor."""
    lo, hi = RANGES[OPS.index(op)]
    return (float(m) / 30) * float(hi - lo) + lo


# ------------------------------------------------------------------ test images, the fixture
def label_map(h, w, seed):
    """19 classes in 5 x 7 blocks with a sprinkle of single pixels: edges for the nearest warps to move."""
    rng = np.random.RandomState(seed)
    blocks = rng.randint(0, 19, ((h + 4) // 5, (w + 6) // 7))
    lab = np.repeat(np.repeat(blocks, 5, 0), 7, 1)[:h, :w].copy()
    lab[rng.rand(h, w) < 0.05] = rng.randint(0, 19)
    return lab.astype(np.uint8)


def levels_image():
    """uint8 [48, 48, 3] of constant 3 x 3 blocks, one grey level per block and channel: where the blend of Sharpness
    against an equal SMOOTH value has to return the byte itself."""
    v = (np.arange(256).reshape(16, 16) * 7 + 3) % 256
    g = np.repeat(np.repeat(v, 3, 0), 3, 1)
    return np.stack([g, (g + 85) % 256, (g * 3) % 256], -1).astype(np.uint8)


def checkerboard(h=24, w=31):
    c = (((np.arange(h)[:, None] + np.arange(w)[None, :]) & 1) * 255).astype(np.uint8)
    return np.stack([c, 255 - c, c], -1)


def load_golden():
    """tests/golden/randaugment_golden.npz (make_golden_randaugment.py) -> the npz and its metadata."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "randaugment_golden.npz"))
    return z, json.loads(str(z["meta"]))
