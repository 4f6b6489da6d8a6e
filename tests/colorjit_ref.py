"""CPU restatement of the reference's ColorJitter chain (transforms/transforms.py:192-362) in numpy, byte for byte what
Pillow computes: ImageEnhance.Brightness / Contrast / Color (Image.blend against black, the rounded mean of L, L of the
pixel) and adjust_hue (RGB -> HSV, H += byte mod 256, HSV -> RGB).  tests/test_colorjitter_cpu.py pins it to live
Pillow over all 2^24 colours and to the fixture recorded from the reference; the GPU tests then need neither.

An image is uint8 [H, W, 3]; a program is a list of (op, value): ("brightness" | "contrast" | "saturation", factor) or
("hue", byte)."""
import json
import os

import numpy as np

OPS = ("brightness", "contrast", "saturation", "hue")       # = SSA_JITTER_* of include/semseg_hip.h
F32 = np.float32


def all_colours():
    """uint8 [4096, 4096, 3]: every RGB colour once (r = y >> 4, g = ((y & 15) << 4) | (x >> 8), b = x & 255)."""
    v = np.arange(1 << 24, dtype=np.uint32).reshape(4096, 4096)
    return np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], -1).astype(np.uint8)


def luma(img):
    c = img.astype(np.int32)                            # 255 * 65536 < 2^31
    return (c[..., 0] * 19595 + c[..., 1] * 38470 + c[..., 2] * 7471 + 0x8000) >> 16


def blend(d, x, f):
    """Image.blend(degenerate, img, f): d broadcastable to x (uint8 values); two separately rounded fp32 operations."""
    f = F32(f)
    d32 = np.asarray(d).astype(F32)
    t = d32 + f * (x.astype(F32) - d32)
    assert t.dtype == F32
    if 0 <= f <= 1:
        return t.astype(np.int32).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.clip(t, 0, 255).astype(np.int32))).astype(np.uint8)


def brightness(img, f):
    return blend(np.zeros((), np.uint8), img, f)


def saturation(img, f):
    return blend(luma(img)[..., None], img, f)


def contrast_mean(img):
    """m = int(S / N + 0.5): S the integer sum of L, the division in double."""
    L = luma(img)
    return int(float(int(L.sum(dtype=np.int64))) / float(L.size) + 0.5)


def contrast(img, f, mean=None):
    return blend(np.full((), contrast_mean(img) if mean is None else mean, np.int64), img, f)


def hue_byte(hue_factor):
    """trunc(hue_factor * 255) mod 256: what np.uint8(hue_factor * 255) gave under NumPy 1.x (-63.75 -> 193)."""
    return int(hue_factor * 255) % 256


def _clip8(v):
    return np.clip(v, 0, 255)


def rgb_to_hsv(img):
    r, g, b = (img[..., i].astype(np.int32) for i in range(3))
    maxc, minc = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
    grey = maxc == minc
    with np.errstate(divide="ignore", invalid="ignore"):
        cr = (maxc - minc).astype(F32)
        s = cr / maxc.astype(F32)
        rc, gc, bc = ((maxc - c).astype(F32) / cr for c in (r, g, b))
        h_r = bc - gc                                                                   # fp32
        h_g = (2.0 + rc.astype(np.float64) - bc.astype(np.float64)).astype(F32)        # double, rounded to fp32
        h_b = (4.0 + gc.astype(np.float64) - rc.astype(np.float64)).astype(F32)
        h = np.where(r == maxc, h_r, np.where(g == maxc, h_g, h_b))
        h = np.where(grey, F32(0), h).astype(F32)
        h = np.fmod(h.astype(np.float64) / 6.0 + 1.0, 1.0).astype(F32)
        H = _clip8((h.astype(np.float64) * 255.0).astype(np.int64))
        S = _clip8((np.where(grey, F32(0), s).astype(np.float64) * 255.0).astype(np.int64))
    H = np.where(grey, 0, H)
    S = np.where(grey, 0, S)
    return np.stack([H, S, maxc], -1).astype(np.uint8)


def hsv_to_rgb(hsv):
    H, S, V = (hsv[..., i].astype(np.int32) for i in range(3))
    hf = H.astype(np.float64) * 6.0 / 255.0
    i = np.floor(hf)
    f = hf - i
    fs = S.astype(np.float64) / 255.0
    v = V.astype(np.float64)

    def rnd(x):
        return _clip8(np.floor(x + 0.5).astype(np.int64))
    p, q, t = rnd(v * (1.0 - fs)), rnd(v * (1.0 - fs * f)), rnd(v * (1.0 - fs * (1.0 - f)))
    k = i.astype(np.int64) % 6
    table = [(V, t, p), (q, V, p), (p, V, t), (p, q, V), (t, p, V), (V, p, q)]
    out = np.stack([np.choose(k, [tab[c] for tab in table]) for c in range(3)], -1)
    return np.where((S == 0)[..., None], V[..., None], out).astype(np.uint8)


def hue(img, byte):
    hsv = rgb_to_hsv(img)
    hsv[..., 0] = (hsv[..., 0].astype(np.int64) + int(byte)) & 255
    return hsv_to_rgb(hsv)


def apply_op(img, op, value):
    return {"brightness": brightness, "contrast": contrast, "saturation": saturation, "hue": hue}[op](img, value)


def jitter(img, program, window=None, flip=False):
    """The program on the crop window (x0, y0, w, h) of img, then the horizontal flip."""
    if window is not None:
        x0, y0, w, h = window
        img = img[y0:y0 + h, x0:x0 + w]
    img = np.ascontiguousarray(img)
    for op, value in program:
        img = apply_op(img, op, value)
    return np.ascontiguousarray(img[:, ::-1]) if flip else img


def get_params(brightness, contrast, saturation, hue):   # noqa: A002  (the reference's argument names)
    """The draws of ColorJitter.get_params from np.random's global generator -> [(op, factor)] in shuffled order (hue
    with its FACTOR, not the byte)."""
    ops = []
    if brightness > 0:
        ops.append(("brightness", np.random.uniform(max(0, 1 - brightness), 1 + brightness)))
    if contrast > 0:
        ops.append(("contrast", np.random.uniform(max(0, 1 - contrast), 1 + contrast)))
    if saturation > 0:
        ops.append(("saturation", np.random.uniform(max(0, 1 - saturation), 1 + saturation)))
    if hue > 0:
        ops.append(("hue", np.random.uniform(-hue, hue)))
    np.random.shuffle(ops)
    return ops


def program_of(draws):
    """[(op, factor)] as drawn -> the program (hue factor -> byte)."""
    return [(op, hue_byte(v) if op == "hue" else float(v)) for op, v in draws]


def pink_image(h, w, seed):
    """A 1/f-like RGB image: white noise shaped by 1/f in the Fourier domain, per channel, stretched to 0..255."""
    rng = np.random.RandomState(seed)
    fy, fx = np.fft.fftfreq(h)[:, None], np.fft.fftfreq(w)[None, :]
    f = np.sqrt(fy * fy + fx * fx)
    f[0, 0] = 1.0
    chans = []
    for _ in range(3):
        x = np.real(np.fft.ifft2(np.fft.fft2(rng.randn(h, w)) / f))
        chans.append((x - x.min()) / (x.max() - x.min()) * 255.0)
    return np.stack(chans, -1).round().astype(np.uint8)


def load_golden():
    """tests/golden/colorjitter_golden.npz (make_golden_colorjitter.py) -> (images [2,37,53,3], outputs [n,37,53,3],
    meta: entries + hashes)."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "colorjitter_golden.npz"))
    return z["images"], z["outputs"], json.loads(str(z["meta"]))
