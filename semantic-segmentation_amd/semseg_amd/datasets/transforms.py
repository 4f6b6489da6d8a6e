"""Label-map resize on the GPU, bit-identical to `mask.resize(size, Image.NEAREST)`
(transforms/joint_transforms.py:193,267,290,319,339,364,466 of the reference).

Pillow's nearest resize walks a double-precision accumulator: the source
coordinate of destination column 0 is scale*0.5 and every further column adds
`scale` to the running sum (ImagingScaleAffine), truncating toward zero.  The
closed form floor((x+0.5)*scale) differs from that in the last bit for some
sizes, so the tables below reproduce the running sum (np.cumsum adds
sequentially, in the same order)."""
import ctypes
import random

import numpy as np
import torch


def nearest_index_table(n_dst, n_src):
    """int32[n_dst]: source index of every destination index (Pillow's rule)."""
    scale = np.float64(n_src) / np.float64(n_dst)
    steps = np.full(n_dst, scale, dtype=np.float64)
    steps[0] = scale * np.float64(0.5)
    pos = np.cumsum(steps)                      # pos[k] = ((scale/2 + scale) + scale) + ...
    idx = np.where(pos < 0, -1, pos.astype(np.int64))
    return np.clip(idx, 0, n_src - 1).astype(np.int32)


_TABLES = {}


def _table(n_dst, n_src, device):
    key = (n_dst, n_src, str(device))
    t = _TABLES.get(key)
    if t is None:
        t = _TABLES[key] = torch.from_numpy(nearest_index_table(n_dst, n_src)).to(device)
    return t


def resize_labels_nearest(mask, size):
    """mask: uint8 CUDA tensor [H,W] or [B,H,W]; size = (Hd, Wd) -> same rank, uint8."""
    from .._lib import lib, check
    assert mask.dtype == torch.uint8 and mask.is_cuda, "label maps are uint8 device tensors"
    squeeze = mask.dim() == 2
    m = mask.unsqueeze(0) if squeeze else mask
    m = m.contiguous()
    B, Hs, Ws = m.shape
    Hd, Wd = int(size[0]), int(size[1])
    out = torch.empty((B, Hd, Wd), dtype=torch.uint8, device=m.device)
    iy, ix = _table(Hd, Hs, m.device), _table(Wd, Ws, m.device)
    check(lib().ssa_resize_nearest_u8(ctypes.c_void_p(m.data_ptr()), B, Hs, Ws, ctypes.c_void_p(out.data_ptr()),
                                      Hd, Wd, ctypes.c_void_p(iy.data_ptr()), ctypes.c_void_p(ix.data_ptr()),
                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
          "ssa_resize_nearest_u8")
    return out[0] if squeeze else out


# ---------------------------------------------------------------------------------------------
# Tail of the image pipeline on the device: crop window + horizontal flip of
# the (image, labels) pair, ToTensor + Normalize on the image, MaskToTensor on the labels
# (datasets/base_loader.py:120-150, transforms/joint_transforms.py:276-281).  The host sends the
# raw uint8 buffers once; what comes back is what `net({'images': ..., 'gts': ...})` consumes.
# ---------------------------------------------------------------------------------------------
MEAN_STD = ([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])      # config.py:96-97 (cfg.DATASET.MEAN / STD)


def crop_flip_normalize(img_u8, labels_u8, window, flip, mean_std=MEAN_STD, jitter=None, blur=None, augment=None):
    """img_u8: uint8 CUDA [H,W,3] (RGB, as np.array(PIL image)); labels_u8: uint8 CUDA [H,W] or None;
    window = (x0, y0, w, h) as PIL's crop box origin + size; flip: mirror the cropped pair.
    jitter: None, or the JitterParams of ColorJitter.get_params -- the image-only augmentation the reference runs
    between the joint transforms and ToTensor (datasets/base_loader.py:141-142), applied to the window in the same
    launch that normalises it (ssa_jitter_luma_sum + ssa_jitter_crop_flip_normalize); the labels do not see it.
    blur: None, or the BlurParams of RandomGaussianBlur.get_params -- the reference's --gblur step, which follows the
    jitter (datasets/__init__.py:102): the window goes through ssa_gblur_crop_flip_normalize instead, which runs the
    jitter program (if any; ssa_jitter_luma_sum first) on the pixels it stages, blurs and normalises in one launch.
    augment: None, or the AugmentParams of RandAugment.get_params -- the reference's --rand_augment step, a JOINT
    transform that runs on the cropped, mirrored pair before the jitter (datasets/__init__.py:83-87): the chain goes
    through ssa_randaug_u8 first, and the jitter (its luma sum taken over the augmented window), the blur, the normalise
    and the label conversion then read what it wrote.  With None nothing changes.
    Returns (image [1,h,w,16] bf16 NHWC -- hand it to the network's trunk --, labels [1,h,w] int64)."""
    from .._lib import lib, check
    assert img_u8.dtype == torch.uint8 and img_u8.is_cuda and img_u8.dim() == 3 and img_u8.shape[2] == 3
    H, W = int(img_u8.shape[0]), int(img_u8.shape[1])
    x0, y0, cw, ch = (int(v) for v in window)
    if labels_u8 is not None:
        assert labels_u8.dtype == torch.uint8 and labels_u8.is_cuda and tuple(labels_u8.shape) == (H, W)
    if augment is not None:       # the pair the later steps read is the augmented window: whole, not mirrored again
        img_u8, labels_u8 = rand_augment(img_u8, labels_u8, augment, (x0, y0, cw, ch), flip)
        H, W, x0, y0, flip = ch, cw, 0, 0, False
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = _image_half(img_u8, (x0, y0, cw, ch), flip, jitter, blur, True, mean_std)
    gts = None
    if labels_u8 is not None:
        labels_u8 = labels_u8.contiguous()
        gts = torch.empty((1, ch, cw), dtype=torch.int64, device=img_u8.device)
        check(lib().ssa_label_u8_crop_flip(ctypes.c_void_p(labels_u8.data_ptr()), H, W, x0, y0, cw, ch,
                                           int(bool(flip)), ctypes.c_void_p(gts.data_ptr()), stream),
              "ssa_label_u8_crop_flip")
    return out, gts


# (blur?, jitter?, normalised output?) -> the entry point.  Both blur entry points take the program as an optional
# argument; a window that is neither jittered nor blurred has no uint8 form.
_IMAGE_ENTRY = {(False, False, True): "ssa_image_u8_crop_flip_normalize",
                (False, True, False): "ssa_jitter_apply_u8", (False, True, True): "ssa_jitter_crop_flip_normalize",
                (True, False, False): "ssa_gblur_u8", (True, False, True): "ssa_gblur_crop_flip_normalize",
                (True, True, False): "ssa_gblur_u8", (True, True, True): "ssa_gblur_crop_flip_normalize"}


def _image_half(img_u8, window, flip, jitter=None, blur=None, normalize=True, mean_std=MEAN_STD):
    """The image half of the tail for every combination: the window (None: the whole image) of img_u8, mirrored under
    `flip`, through the jitter program (JitterParams or None), the blur (BlurParams, a bare sigma or None) and, under
    `normalize`, ToTensor + Normalize -> [1,h,w,16] in the activation type, else uint8 [h,w,3].  One launch, after the
    luma sum where the program has a contrast step; the mean itself is formed on the device: nothing here waits."""
    from .. import hip_backend as hb
    from .._lib import lib, check
    if blur is not None and not isinstance(blur, BlurParams):
        blur = BlurParams(blur)
    if jitter is not None and not isinstance(jitter, JitterParams):
        raise TypeError("jitter parameters must be a JitterParams (ColorJitter.get_params), not %r" % type(jitter))
    if img_u8.dtype != torch.uint8 or img_u8.dim() != 3 or img_u8.shape[2] != 3:
        raise ValueError("the image must be uint8 [H, W, 3]")
    img_u8 = img_u8.contiguous()
    H, W = int(img_u8.shape[0]), int(img_u8.shape[1])
    x0, y0, cw, ch = (0, 0, W, H) if window is None else (int(v) for v in window)
    if not (cw > 0 and ch > 0 and x0 >= 0 and y0 >= 0 and x0 + cw <= W and y0 + ch <= H):
        raise ValueError("window %r is empty or not inside the %d x %d image" % ((x0, y0, cw, ch), W, H))
    name = _IMAGE_ENTRY[blur is not None, jitter is not None, bool(normalize)]
    args = [hb._p(img_u8), H, W, x0, y0, cw, ch, int(bool(flip))]
    if jitter is not None:
        pg, counter = jitter.program(), None
        if "contrast" in jitter.order:
            counter = torch.empty((1,), dtype=torch.int64, device=img_u8.device)
            check(lib().ssa_jitter_luma_sum(*args[:7], ctypes.byref(pg), hb._p(counter), hb._s()), "ssa_jitter_luma_sum")
        args += [ctypes.byref(pg), hb._p(counter)]
    elif blur is not None:
        args += [None, None]
    if blur is not None:
        args += [ctypes.byref(blur.taps()), hb._p(_gblur_lut(img_u8.device))]
    if normalize:
        out = torch.empty((1, ch, cw, 16), dtype=hb.ACT_DTYPE, device=img_u8.device)
        args += [(ctypes.c_float * 3)(*mean_std[0]), (ctypes.c_float * 3)(*mean_std[1]), hb._p(out), 16]
    else:
        out = torch.empty((ch, cw, 3), dtype=torch.uint8, device=img_u8.device)
        args.append(hb._p(out))
    check(getattr(lib(), name)(*args, hb._s()), name)
    return out


# ---------------------------------------------------------------------------------------------
# The scale step on the device: `img.resize((w, h), Image.BICUBIC)` (transforms/joint_transforms.py:
# 433-471 and the Scale / ResizeHeight transforms), bit-identical to Pillow.  Pillow resamples 8-bit
# images in two passes with 22-bit fixed-point taps (libImaging/Resample.c); the tap tables are
# derived here in double precision, operation by operation as precompute_coeffs /
# normalize_coeffs_8bpc do, and the two integer passes run on the GPU (ssa_resample_u8).
# ---------------------------------------------------------------------------------------------
def bicubic_tables(n_dst, n_src):
    """-> (ksize, bounds int32 [n_dst, 2] = (first, count), coefs int32 [n_dst, ksize])."""
    scale = np.float64(n_src) / np.float64(n_dst)
    fscale = scale if scale >= 1.0 else np.float64(1.0)
    support = np.float64(2.0) * fscale
    ksize = int(np.ceil(support)) * 2 + 1
    center = np.float64(0.0) + (np.arange(n_dst, dtype=np.float64) + 0.5) * scale
    ss = np.float64(1.0) / fscale
    first = np.maximum((center - support + 0.5).astype(np.int64), 0)          # (int) truncates; values >= -0.5 here
    first = np.where(center - support + 0.5 < 0, 0, first)
    last = np.minimum((center + support + 0.5).astype(np.int64), n_src)
    count = last - first
    j = np.arange(ksize, dtype=np.int64)[None, :]
    x = (j + first[:, None] - center[:, None] + 0.5) * ss
    ax = np.abs(x)
    a = np.float64(-0.5)
    w = np.where(ax < 1.0, ((a + 2.0) * ax - (a + 3.0)) * ax * ax + 1,
                 np.where(ax < 2.0, (((ax - 5) * ax + 8) * ax - 4) * a, 0.0))
    w = np.where(j < count[:, None], w, 0.0)
    ww = np.zeros(n_dst, dtype=np.float64)
    for k in range(ksize):                       # the C loop adds the taps in order
        ww = ww + w[:, k]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    fixed = np.where(w < 0, (-0.5 + w * float(1 << 22)).astype(np.int64), (0.5 + w * float(1 << 22)).astype(np.int64))
    fixed = np.where(j < count[:, None], fixed, 0)
    return ksize, np.stack([first, count], 1).astype(np.int32), fixed.astype(np.int32)


_BICUBIC = {}


def _bicubic(n_dst, n_src, device):
    key = (n_dst, n_src, str(device))
    t = _BICUBIC.get(key)
    if t is None:
        ksize, bounds, coefs = bicubic_tables(n_dst, n_src)
        t = _BICUBIC[key] = (ksize, torch.from_numpy(bounds).to(device), torch.from_numpy(coefs).to(device))
    return t


def resize_image_bicubic(img_u8, size):
    """img_u8: uint8 CUDA [H,W,C] (as np.array(PIL image)); size = (Hd, Wd) -> uint8 [Hd,Wd,C], bit-identical to
    `Image.fromarray(img).resize((Wd, Hd), Image.BICUBIC)`."""
    from .._lib import lib, check
    assert img_u8.dtype == torch.uint8 and img_u8.is_cuda and img_u8.dim() == 3
    cur = img_u8.contiguous()
    Hd, Wd = int(size[0]), int(size[1])
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for axis, n_out in ((1, Wd), (0, Hd)):       # horizontal pass first, then vertical (ImagingResampleInner)
        Hs, Ws, C = (int(v) for v in cur.shape)
        if n_out == (Ws if axis else Hs):
            continue
        ksize, bounds, coefs = _bicubic(n_out, Ws if axis else Hs, cur.device)
        out = torch.empty((Hs, n_out, C) if axis else (n_out, Ws, C), dtype=torch.uint8, device=cur.device)
        check(lib().ssa_resample_u8(ctypes.c_void_p(cur.data_ptr()), Hs, Ws, C, axis, ctypes.c_void_p(out.data_ptr()),
                                    n_out, ctypes.c_void_p(bounds.data_ptr()), ctypes.c_void_p(coefs.data_ptr()), ksize,
                                    stream), "ssa_resample_u8")
        cur = out
    return cur


# ---------------------------------------------------------------------------------------------
# ColorJitter on the device (transforms/transforms.py:192-362; datasets/__init__.py:94-99 builds
# ColorJitter(0.25, 0.25, 0.25, 0.25) under the default --color_aug): ImageEnhance.Brightness / Contrast / Color
# and the HSV round trip of adjust_hue, bit-identical to Pillow (csrc/color_jitter.hip).  The random draws stay on
# the host and consume np.random exactly as the reference does; what travels to the kernels is the drawn program.
# ---------------------------------------------------------------------------------------------
JITTER_OPS = ("brightness", "contrast", "saturation", "hue")      # index = SSA_JITTER_* of include/semseg_hip.h


def hue_to_byte(hue_factor):
    """The byte adjust_hue adds to H: the reference writes np.uint8(hue_factor * 255), which under the NumPy 1.x it
    was written for truncates toward zero and wraps modulo 256 (-63.75 -> 193); NumPy 2 raises OverflowError for a
    negative factor instead.  This is the NumPy 1.x value."""
    return int(hue_factor * 255) % 256


class JitterParams:
    """One drawn ColorJitter transform: `order` = the enabled operations in application order (names of
    JITTER_OPS), the three blend factors, the hue factor and the byte it becomes."""
    __slots__ = ("order", "brightness", "contrast", "saturation", "hue", "hue_byte")

    def __init__(self, order=(), brightness=1.0, contrast=1.0, saturation=1.0, hue=0.0, hue_byte=None):
        self.order = tuple(order)
        self.brightness, self.contrast, self.saturation, self.hue = (float(brightness), float(contrast),
                                                                     float(saturation), float(hue))
        self.hue_byte = hue_to_byte(self.hue) if hue_byte is None else int(hue_byte)
        if any(op not in JITTER_OPS for op in self.order) or len(set(self.order)) != len(self.order):
            raise ValueError("JitterParams: order must hold distinct names of %s, not %r" % (JITTER_OPS, self.order))
        if not 0 <= self.hue_byte <= 255:
            raise ValueError("JitterParams: hue_byte must be in 0..255")

    def __repr__(self):
        return "JitterParams(order=%r, brightness=%r, contrast=%r, saturation=%r, hue=%r, hue_byte=%r)" % (
            self.order, self.brightness, self.contrast, self.saturation, self.hue, self.hue_byte)

    def program(self):
        """-> the ssa_jitter_program the kernels take by value."""
        from .._lib import JitterProgram
        pg = JitterProgram()
        pg.n_ops = len(self.order)
        for k, op in enumerate(self.order):
            pg.op[k] = JITTER_OPS.index(op)
        pg.factor[0], pg.factor[1], pg.factor[2] = self.brightness, self.contrast, self.saturation
        pg.hue_byte = self.hue_byte
        return pg


def color_jitter(img_u8, params, window=None, flip=False):
    """img_u8: uint8 CUDA [H,W,3]; params: JitterParams; window = (x0, y0, w, h) or None for the whole image; flip:
    mirror the result.  -> uint8 [h,w,3] = the drawn transform applied to the cropped image, as
    ColorJitter.get_params(...)(img.crop(...)) followed by FLIP_LEFT_RIGHT gives it (the contrast mean is taken over
    the window and does not depend on the flip)."""
    if not isinstance(params, JitterParams):
        raise TypeError("jitter parameters must be a JitterParams (ColorJitter.get_params), not %r" % type(params))
    return _image_half(img_u8, window, flip, params, None, False)


def adjust_brightness(img_u8, brightness_factor):
    """transforms/transforms.py:192-209 (ImageEnhance.Brightness) on a uint8 CUDA [H,W,3] image."""
    return color_jitter(img_u8, JitterParams(("brightness",), brightness=brightness_factor))


def adjust_contrast(img_u8, contrast_factor):
    """transforms/transforms.py:212-229 (ImageEnhance.Contrast)."""
    return color_jitter(img_u8, JitterParams(("contrast",), contrast=contrast_factor))


def adjust_saturation(img_u8, saturation_factor):
    """transforms/transforms.py:232-249 (ImageEnhance.Color)."""
    return color_jitter(img_u8, JitterParams(("saturation",), saturation=saturation_factor))


def adjust_hue(img_u8, hue_factor):
    """transforms/transforms.py:252-294: H of the HSV image shifted by hue_to_byte(hue_factor), modulo 256."""
    if not (-0.5 <= hue_factor <= 0.5):
        raise ValueError("hue_factor is not in [-0.5, 0.5].")
    return color_jitter(img_u8, JitterParams(("hue",), hue=hue_factor))


class ColorJitter:
    """transforms/transforms.py:297-362 for uint8 CUDA [H,W,3] images: the same constructor, the same draws from
    np.random's global generator in the same order, the drawn transform applied on the device."""

    def __init__(self, brightness=0, contrast=0, saturation=0, hue=0):
        self.brightness = brightness
        self.contrast = contrast
        self.saturation = saturation
        self.hue = hue

    @staticmethod
    def get_params(brightness, contrast, saturation, hue):
        """One np.random.uniform per enabled operation (brightness, contrast, saturation, hue, in that order), then
        np.random.shuffle of the list of enabled operations -> JitterParams."""
        factors, order = {}, []
        if brightness > 0:
            factors["brightness"] = np.random.uniform(max(0, 1 - brightness), 1 + brightness)
            order.append("brightness")
        if contrast > 0:
            factors["contrast"] = np.random.uniform(max(0, 1 - contrast), 1 + contrast)
            order.append("contrast")
        if saturation > 0:
            factors["saturation"] = np.random.uniform(max(0, 1 - saturation), 1 + saturation)
            order.append("saturation")
        if hue > 0:
            factors["hue"] = np.random.uniform(-hue, hue)
            order.append("hue")
        np.random.shuffle(order)        # a list of n entries: the same n - 1 draws whatever it holds
        return JitterParams(order, **factors)

    def __call__(self, img_u8):
        return color_jitter(img_u8, self.get_params(self.brightness, self.contrast, self.saturation, self.hue))


# ---------------------------------------------------------------------------------------------
# RandomGaussianBlur on the device (transforms/transforms.py:154-162; datasets/__init__.py:102 appends it under
# --gblur, after ColorJitter): skimage.filters.gaussian(np.array(img), sigma, multichannel=True) * 255 truncated to
# uint8, bit-identical to SciPy's arithmetic (csrc/gblur.hip).  skimage's function is a wrapper: it converts the bytes
# to float64 (byte_to_float64() below -- the ONE place where that conversion is stated) and calls
# scipy.ndimage.gaussian_filter(image, [sigma, sigma, 0], mode='nearest', truncate=4.0).  The draw stays on the host
# and consumes Python's `random` as the reference does; what travels to the kernel is the tap table.
# ---------------------------------------------------------------------------------------------
def byte_to_float64():
    """float64[256]: what skimage's img_as_float makes of a uint8 image (skimage/util/dtype.py: np.multiply(image,
    1. / 255, dtype=float64)).  It is a product by the rounded reciprocal, not a division: 24 of the 256 values differ
    from b / 255 in the last bit."""
    return np.multiply(np.arange(256, dtype=np.uint8), 1 / 255, dtype=np.float64)


def gaussian_taps(sigma):
    """-> (radius, float64[radius + 1]): the radius int(4 sigma + 0.5) of scipy.ndimage.gaussian_filter1d at
    truncate=4.0 and the normalised weights at distance 0..radius, derived operation by operation as
    scipy.ndimage._gaussian_kernel1d derives them (the kernel is symmetric: SciPy's reversal changes nothing).
    ValueError when the radius is outside 1..5, i.e. for sigma outside about [0.125, 1.375): the reference draws
    sigma from [0.15, 1.3)."""
    sigma = float(sigma)
    if not np.isfinite(sigma) or sigma <= 0:
        raise ValueError("gaussian_taps: sigma must be positive and finite, not %r" % sigma)
    radius = int(4.0 * sigma + 0.5)
    if not 1 <= radius <= 5:
        raise ValueError("gaussian_taps: sigma %r gives the radius %d; the device blur covers 1..5" % (sigma, radius))
    sigma2 = sigma * sigma
    x = np.arange(-radius, radius + 1)
    phi_x = np.exp(-0.5 / sigma2 * x ** 2)
    phi_x = phi_x / phi_x.sum()
    return radius, np.ascontiguousarray(phi_x[radius:], dtype=np.float64)


class BlurParams:
    """One drawn RandomGaussianBlur: sigma, and the radius and weights it means."""
    __slots__ = ("sigma", "radius", "weights")

    def __init__(self, sigma):
        self.sigma = float(sigma)
        self.radius, self.weights = gaussian_taps(self.sigma)

    def __repr__(self):
        return "BlurParams(sigma=%r)" % self.sigma

    def taps(self):
        """-> the ssa_gblur_taps the kernel takes by value."""
        from .._lib import GblurTaps
        tp = GblurTaps()
        tp.radius = self.radius
        for j, w in enumerate(self.weights):
            tp.w[j] = float(w)
        return tp


_GBLUR_LUT = {}


def _gblur_lut(device):
    key = str(device)
    t = _GBLUR_LUT.get(key)
    if t is None:
        t = _GBLUR_LUT[key] = torch.from_numpy(byte_to_float64()).to(device)
    return t


def gaussian_blur(img_u8, sigma_or_params, window=None, flip=False, jitter=None):
    """img_u8: uint8 CUDA [H,W,3]; sigma_or_params: sigma or BlurParams; window = (x0, y0, w, h) or None for the whole
    image; flip: mirror; jitter: None or the JitterParams to apply first.  -> uint8 [h,w,3] = what the reference's
    RandomGaussianBlur makes, at that sigma, of the cropped (mirrored, jittered) image: the blur sees the WINDOW's
    edges, not the source's."""
    return _image_half(img_u8, window, flip, jitter, sigma_or_params, False)


class RandomGaussianBlur:
    """transforms/transforms.py:154-162 for uint8 CUDA [H,W,3] images: the same single draw from Python's `random`, the
    blur on the device."""

    @staticmethod
    def get_params():
        """sigma = 0.15 + random.random() * 1.15 -> BlurParams."""
        return BlurParams(0.15 + random.random() * 1.15)

    def __call__(self, img_u8):
        return gaussian_blur(img_u8, self.get_params())


# ---------------------------------------------------------------------------------------------
# RandAugment on the device (datasets/randaugment.py; datasets/__init__.py:83-87 inserts RandAugment(N, M) under
# --rand_augment N,M after RandomSizeAndCrop and RandomHorizontallyFlip): a JOINT transform of the cropped, mirrored
# (image, labels) pair -- N operations drawn from the 14 of augment_list, each bit-identical to the Pillow call the
# reference makes (csrc/randaugment.hip).  The draws stay on the host and consume Python's `random` as the reference
# does; what travels to the kernels is the drawn program.
# ---------------------------------------------------------------------------------------------
RANDAUG_OPS = ("Identity", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "AutoContrast", "Invert",
               "Equalize", "Solarize", "Posterize", "Color", "Brightness", "Sharpness")   # index = SSA_RANDAUG_*
# augment_list's (minval, maxval), datasets/randaugment.py:179-201
RANDAUG_RANGES = ((0., 1.0), (0., 0.3), (0., 0.3), (0., 0.33), (0., 0.33), (0, 30), (0, 1), (0, 1), (0, 1), (0, 110),
                  (4, 8), (0.1, 1.9), (0.1, 1.9), (0.1, 1.9))
RANDAUG_GEOMETRIC = RANDAUG_OPS[1:6]              # the operations that draw a sign and move the labels
RANDAUG_MAX_OPS = 8                               # SSA_RANDAUG_MAX_OPS


def rotate_matrix(angle, w, h):
    """The six coefficients Image.rotate(angle) hands to Image.transform for a w x h image (no centre, no translation,
    no expansion; angle % 360 != 0): the rounded rotation about (w / 2, h / 2), operation by operation as Pillow's
    Python code derives it."""
    import math
    angle = -math.radians(angle % 360.0)
    m = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0,
         round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]
    cx, cy = w / 2.0, h / 2.0
    x, y = -cx, -cy
    m[2], m[5] = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
    m[2] += cx
    m[5] += cy
    return m


class AugmentParams:
    """One drawn RandAugment chain: `ops` = [(name of RANDAUG_OPS, signed value)] in application order -- the shear, the
    translation in PIXELS, the angle in degrees, the Solarize threshold, the Posterize bits (int), the blend factor; unused
    where the operation has no magnitude -- and `size` = (w, h) of the image the operations see."""
    __slots__ = ("ops", "size")

    def __init__(self, ops, size):
        self.ops = [(str(op), int(v) if op == "Posterize" else float(v)) for op, v in ops]
        self.size = (int(size[0]), int(size[1]))
        if any(op not in RANDAUG_OPS for op, _ in self.ops):
            raise ValueError("AugmentParams: operations must be names of %s, not %r" % (RANDAUG_OPS, self.ops))
        if len(self.ops) > RANDAUG_MAX_OPS:
            raise ValueError("AugmentParams: at most %d operations, not %d" % (RANDAUG_MAX_OPS, len(self.ops)))
        if any(op == "Posterize" and not 4 <= v <= 8 for op, v in self.ops):
            raise ValueError("AugmentParams: Posterize keeps 4..8 bits")
        if self.size[0] <= 0 or self.size[1] <= 0:
            raise ValueError("AugmentParams: size must be positive, not %r" % (self.size,))

    def __repr__(self):
        return "AugmentParams(%r, size=%r)" % (self.ops, self.size)

    def histograms(self):
        """How many operations of the chain need a histogram of the image."""
        return sum(op in ("AutoContrast", "Equalize") for op, _ in self.ops)

    def matrix(self, k):
        """The affine coefficients of the k-th operation (zeros where it is not geometric or is a copy)."""
        op, v = self.ops[k]
        w, h = self.size
        if op == "ShearX":
            return [1.0, v, 0.0, 0.0, 1.0, 0.0]
        if op == "ShearY":
            return [1.0, 0.0, 0.0, v, 1.0, 0.0]
        if op == "TranslateX":
            return [1.0, 0.0, v, 0.0, 1.0, 0.0]
        if op == "TranslateY":
            return [1.0, 0.0, 0.0, 0.0, 1.0, v]
        if op == "Rotate" and v % 360.0 != 0:
            return rotate_matrix(v, w, h)
        return [0.0] * 6

    def program(self):
        """-> the ssa_randaug_program the entry point takes."""
        from .._lib import RandaugProgram
        pg = RandaugProgram()
        pg.n_ops = len(self.ops)
        for k, (op, v) in enumerate(self.ops):
            pg.op[k] = RANDAUG_OPS.index(op)
            pg.value[k] = float(v)
            for j, c in enumerate(self.matrix(k)):
                pg.matrix[k][j] = float(c)
        return pg


def rand_augment(img_u8, labels_u8, params, window=None, flip=False, ignore_label=255):
    """img_u8: uint8 CUDA [H,W,3]; labels_u8: uint8 CUDA [H,W] or None; params: AugmentParams drawn for the window's size;
    window = (x0, y0, w, h) or None for the whole image; flip: mirror the pair first.  -> (uint8 [h,w,3], uint8 [h,w] or
    None) = the drawn chain applied to the cropped, mirrored pair as the reference's RandAugment.__call__ applies it.
    Only the five geometric operations touch the labels; ignore_label is the reference's fillmask
    (cfg.DATASET.IGNORE_LABEL), the image fill is (0, 0, 0).  One call of ssa_randaug_u8: the histograms and tables of
    AutoContrast / Equalize stay on the device, nothing here waits for it."""
    from .. import hip_backend as hb
    from .._lib import lib, check
    if not isinstance(params, AugmentParams):
        raise TypeError("augment parameters must be an AugmentParams (RandAugment.get_params), not %r" % type(params))
    if img_u8.dtype != torch.uint8 or img_u8.dim() != 3 or img_u8.shape[2] != 3:
        raise ValueError("the image must be uint8 [H, W, 3]")
    img_u8 = img_u8.contiguous()
    H, W = int(img_u8.shape[0]), int(img_u8.shape[1])
    x0, y0, cw, ch = (0, 0, W, H) if window is None else (int(v) for v in window)
    if not (cw > 0 and ch > 0 and x0 >= 0 and y0 >= 0 and x0 + cw <= W and y0 + ch <= H):
        raise ValueError("window %r is empty or not inside the %d x %d image" % ((x0, y0, cw, ch), W, H))
    if params.size != (cw, ch):
        raise ValueError("the parameters were drawn for a %d x %d image, the window is %d x %d" % (params.size + (cw, ch)))
    if labels_u8 is not None:
        if labels_u8.dtype != torch.uint8 or tuple(labels_u8.shape) != (H, W):
            raise ValueError("the labels must be uint8 [H, W] of the image's size")
        labels_u8 = labels_u8.contiguous()
    dev = img_u8.device
    out = torch.empty((ch, cw, 3), dtype=torch.uint8, device=dev)
    tmp = torch.empty_like(out)
    lab_out = lab_tmp = None
    if labels_u8 is not None:
        lab_out = torch.empty((ch, cw), dtype=torch.uint8, device=dev)
        lab_tmp = torch.empty_like(lab_out)
    nh = params.histograms()
    hist = torch.zeros((nh * 768,), dtype=torch.int32, device=dev) if nh else None    # cleared in stream order
    pg = params.program()
    check(lib().ssa_randaug_u8(hb._p(img_u8), hb._p(labels_u8), H, W, x0, y0, cw, ch, int(bool(flip)), ctypes.byref(pg),
                               int(ignore_label), hb._p(hist), hb._p(out), hb._p(tmp), hb._p(lab_out), hb._p(lab_tmp),
                               hb._s()), "ssa_randaug_u8")
    return out, lab_out


class RandAugment:
    """datasets/randaugment.py:250-263 for uint8 CUDA buffers: the same constructor, the same draws from Python's
    `random` in the same order, the drawn chain applied on the device."""

    def __init__(self, n, m):
        self.n = n
        self.m = m      # [0, 30]

    def get_params(self, size):
        """size = (w, h) of the image the operations will see.  random.choices of n entries of augment_list, then, walking
        them in order, one random.random() for each of ShearX, ShearY, TranslateX, TranslateY, Rotate (the value is
        negated when the draw is > 0.5); the others draw nothing -> AugmentParams.  The generator is left in the state the
        reference's RandAugment(n, m)(img, mask) leaves it in.  m outside [0, 30] fails the reference's asserts."""
        if not 0 <= self.m <= 30:
            raise ValueError("RandAugment: the magnitude m must be in [0, 30], not %r" % (self.m,))
        w, h = int(size[0]), int(size[1])
        chosen = random.choices(range(len(RANDAUG_OPS)), k=self.n)
        ops = []
        for i in chosen:
            op, (minval, maxval) = RANDAUG_OPS[i], RANDAUG_RANGES[i]
            val = (float(self.m) / 30) * float(maxval - minval) + minval
            if op in RANDAUG_GEOMETRIC:
                if random.random() > 0.5:
                    val = -val
                if op == "TranslateX":
                    val = val * w
                elif op == "TranslateY":
                    val = val * h
            elif op == "Posterize":
                val = int(val)
            ops.append((op, val))
        return AugmentParams(ops, (w, h))

    def __call__(self, img_u8, labels_u8):
        return rand_augment(img_u8, labels_u8, self.get_params((int(img_u8.shape[1]), int(img_u8.shape[0]))))


class DevicePrefetcher:
    """H2D overlap for the input pipeline (datasets/base_loader.py:120-150 hands CPU tensors to
    train.py:487, which copies them synchronously): wraps any iterable of (images, gts, ...) batches, keeps
    ONE batch in flight -- pinned host staging + non-blocking copies on a side stream -- and yields device
    tensors whose readiness the consumer stream waits on.  Non-tensor entries pass through."""

    def __init__(self, loader, device="cuda"):
        self.loader, self.device = loader, torch.device(device)
        self.stream = torch.cuda.Stream(self.device) if self.device.type == "cuda" else None

    def __len__(self):
        return len(self.loader)

    def _stage(self, batch):
        if self.stream is None:
            return batch, None
        with torch.cuda.stream(self.stream):
            out = tuple(t.pin_memory().to(self.device, non_blocking=True) if torch.is_tensor(t) else t for t in batch)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        return out, ev

    def __iter__(self):
        it = iter(self.loader)
        try:
            nxt = self._stage(next(it))
        except StopIteration:
            return
        while nxt is not None:
            cur, ev = nxt
            try:
                nxt = self._stage(next(it))       # the next batch's copy runs under this batch's compute
            except StopIteration:
                nxt = None
            if ev is not None:
                torch.cuda.current_stream(self.device).wait_event(ev)
                for t in cur:
                    if torch.is_tensor(t):
                        t.record_stream(torch.cuda.current_stream(self.device))
            yield cur


# ---------------------------------------------------------------------------------------------
# Boundary label relaxation (transforms/transforms.py:74-123): the [C+1,H,W] multi-hot target of
# --jointwtborder from a label map that is already on the device.  The training path does not go
# through here -- ImgWtLossSoftNLL relaxes the int64 labels of crop_flip_normalize itself and never
# materialises this tensor; the class is for users who want the tensor.
class RelaxedBoundaryLossToTensor(object):
    """Device label map, uint8 or int64, [H,W] or [B,H,W] -> uint8 [C+1,H,W] or [B,C+1,H,W]: channel c of a pixel is 1
    iff a pixel of its (2*cfg.BORDER_WINDOW+1)^2 window has label c; `ignore_id`, labels outside [0, C) and positions
    outside the image are the extra channel C; pixels whose own label is in cfg.STRICTBORDERCLASS keep its one-hot."""

    def __init__(self, ignore_id, num_classes):
        self.ignore_id = ignore_id
        self.num_classes = num_classes

    def __call__(self, img):
        from .. import hip_backend as hb
        from ..config import cfg
        if cfg.REDUCE_BORDER_EPOCH != -1 and cfg.EPOCH > cfg.REDUCE_BORDER_EPOCH:
            raise NotImplementedError("the reduced-border mode (--rlx_off_epoch, cfg.EPOCH > cfg.REDUCE_BORDER_EPOCH) "
                                      "is not on the accelerated path")
        assert torch.is_tensor(img) and img.dim() in (2, 3), "a label map [H,W] or [B,H,W] on the device"
        squeeze = img.dim() == 2
        sets, _ = hb.relax_class_sets(img.unsqueeze(0) if squeeze else img, self.num_classes, self.ignore_id,
                                      cfg.BORDER_WINDOW, cfg.STRICTBORDERCLASS)
        out = hb.relax_multihot(sets, self.num_classes)
        return out[0] if squeeze else out


# ---------------------------------------------------------------------------------------------
# RandomSizeAndCrop (transforms/joint_transforms.py:433-471 over RandomCrop, joint_transforms.py:73-181): the first joint
# transform of every training recipe, and the one that places the crop over the centroid of a class-uniform item
# (datasets/base_loader.py:129-132).  The draws stay on the host and consume Python's `random` exactly as the
# reference does; what they decide travels as a CropPlan, and the device resizes, pads (only where the plan says so:
# ssa_pad_u8) and hands crop_flip_normalize its window.
# ---------------------------------------------------------------------------------------------
class CropPlan:
    """What one call of the reference's RandomSizeAndCrop decided.
    scale_amt: the drawn scale (times the pre_size scale), what the reference appends to its result;
    size = (w, h) of the resized pair; border = (pad_w, pad_h) of ImageOps.expand, each on both sides (joint_transforms.py:
    165-177); margins = (left, top, right, bottom) of add_margin (TRANSLATE_AUG_FIX, joint_transforms.py:126-141);
    window = (x0, y0, w, h) of the crop inside the resized and padded pair; centroid: the scaled centroid or None."""

    def __init__(self, scale_amt, size, border, margins, window, centroid):
        self.scale_amt, self.size, self.border, self.margins = scale_amt, tuple(size), tuple(border), tuple(margins)
        self.window, self.centroid = tuple(window), None if centroid is None else tuple(centroid)

    @property
    def pad(self):
        """(left, top, right, bottom) the device adds around the resized pair."""
        (bw, bh), (l, t, r, b) = self.border, self.margins
        return (bw + l, bh + t, bw + r, bh + b)

    def __repr__(self):
        return "CropPlan(scale_amt=%r, size=%r, border=%r, margins=%r, window=%r, centroid=%r)" % (
            self.scale_amt, self.size, self.border, self.margins, self.window, self.centroid)


def pad_u8(src_u8, pad, fill):
    """src_u8: uint8 device tensor [H,W] or [H,W,3]; pad = (left, top, right, bottom); fill: an int or three ->
    the padded copy, what ImageOps.expand / add_margin give for L and RGB images."""
    from .. import hip_backend as hb
    from .._lib import lib, check
    if src_u8.dtype != torch.uint8 or not (src_u8.dim() == 2 or (src_u8.dim() == 3 and src_u8.shape[2] == 3)):
        raise ValueError("uint8 [H,W] or [H,W,3]")
    src_u8 = src_u8.contiguous()
    H, W = int(src_u8.shape[0]), int(src_u8.shape[1])
    ch = 1 if src_u8.dim() == 2 else 3
    left, top, right, bottom = (int(v) for v in pad)
    fill3 = bytes([int(fill)] * 3 if isinstance(fill, int) else [int(v) for v in fill])
    out = torch.empty((H + top + bottom, W + left + right) + tuple(src_u8.shape[2:]), dtype=torch.uint8,
                      device=src_u8.device)
    check(lib().ssa_pad_u8(hb._p(src_u8), H, W, ch, left, top, right, bottom, fill3, hb._p(out), hb._s()), "ssa_pad_u8")
    return out


class RandomSizeAndCrop(object):
    """transforms/joint_transforms.py:433-471 for uint8 device buffers: the same constructor, the same draws from Python's
    `random` in the same order.  get_params draws; apply runs the plan on the device."""

    def __init__(self, crop_size, crop_nopad, scale_min=0.5, scale_max=2.0, full_size=False, pre_size=None):
        from ..config import cfg
        if isinstance(crop_size, (list, tuple)):
            self.size = tuple(crop_size)                # (h, w)
        else:
            self.size = (int(crop_size), int(crop_size))
        self.nopad = crop_nopad
        self.ignore_index = cfg.DATASET.IGNORE_LABEL    # read at construction, as RandomCrop does
        self.pad_color = (0, 0, 0)
        self.scale_min, self.scale_max = scale_min, scale_max
        self.full_size, self.pre_size = full_size, pre_size

    @staticmethod
    def _crop_in_image(centroid, target_w, target_h, w, h):
        """joint_transforms.py:101-121 -> (x1, y1)."""
        if centroid is not None:                        # the crop covers the centroid and stays inside the image
            c_x, c_y = centroid
            x1 = min(w - target_w, max(0, random.randint(c_x - target_w, c_x)))
            y1 = min(h - target_h, max(0, random.randint(c_y - target_h, c_y)))
        else:                                           # an axis that fits exactly draws nothing
            x1 = 0 if w == target_w else random.randint(0, w - target_w)
            y1 = 0 if h == target_h else random.randint(0, h - target_h)
        return x1, y1

    def get_params(self, size, centroid=None):
        """size = (w, h) of the pair, centroid = (x, y) of a class-uniform item or None -> CropPlan.  Python's `random`
        is left in the state RandomSizeAndCrop.__call__ leaves it in: one uniform() for the scale, then RandomCrop's
        draws -- none when the resized pair already has the crop's size.  As in the reference, the centroid is scaled
        but NOT moved by a border the crop adds.  A plan whose window does not lie inside the padded pair (the reference
        reaches one under TRANSLATE_AUG_FIX when only one side is shorter than the crop, and lets Pillow fill the rest
        with zeros) raises ValueError after the draws."""
        from ..config import cfg
        in_w, in_h = int(size[0]), int(size[1])
        scale_amt = random.uniform(self.scale_min, self.scale_max)
        if self.pre_size is not None:
            scale_amt *= self.pre_size / (in_w if in_w > in_h else in_h)
        if self.full_size:
            self.size = (in_h, in_w)
        w, h = int(in_w * scale_amt), int(in_h * scale_amt)
        if centroid is not None:
            centroid = [int(c * scale_amt) for c in centroid]
        resized = (w, h)
        target_h, target_w = self.size
        border, margins = (0, 0), (0, 0, 0, 0)
        if w == target_w and h == target_h:
            x1, y1 = 0, 0
        elif cfg.DATASET.TRANSLATE_AUG_FIX and w < target_w and h < target_h:
            left = random.randint(0, target_w - w)      # the image slides inside the crop
            top = random.randint(0, target_h - h)
            margins = (left, top, target_w - w - left, target_h - h - top)
            x1, y1 = 0, 0
        else:
            if cfg.DATASET.TRANSLATE_AUG_FIX:
                pass
            elif self.nopad:
                if target_h > h or target_w > w:
                    target_h = target_w = min(w, h)
            else:
                pad_h = (target_h - h) // 2 + 1 if target_h > h else 0
                pad_w = (target_w - w) // 2 + 1 if target_w > w else 0
                border = (pad_w, pad_h)
                w, h = w + 2 * pad_w, h + 2 * pad_h
            x1, y1 = self._crop_in_image(centroid, target_w, target_h, w, h)
        plan = CropPlan(scale_amt, resized, border, margins, (x1, y1, target_w, target_h), centroid)
        l, t, r, b = plan.pad
        if not (x1 >= 0 and y1 >= 0 and x1 + target_w <= resized[0] + l + r and y1 + target_h <= resized[1] + t + b):
            raise ValueError("%r: the crop window is not inside the %d x %d pair" % (plan, resized[0] + l + r,
                                                                                     resized[1] + t + b))
        return plan

    def apply(self, plan, img_u8_cuda, labels_u8_cuda):
        """The plan on the device: bicubic / nearest resize of the pair to plan.size, then -- only where the plan has a
        border or margins -- the constant padding (image (0, 0, 0), labels the ignore label).  -> (img, labels, window):
        what crop_flip_normalize(img, labels, window, flip, ...) takes."""
        w, h = plan.size
        img = resize_image_bicubic(img_u8_cuda, (h, w))
        labels = resize_labels_nearest(labels_u8_cuda, (h, w))
        if any(plan.pad):
            img = pad_u8(img, plan.pad, self.pad_color)
            labels = pad_u8(labels, plan.pad, self.ignore_index)
        return img, labels, plan.window

    def __call__(self, img_u8_cuda, labels_u8_cuda, centroid=None):
        plan = self.get_params((int(img_u8_cuda.shape[1]), int(img_u8_cuda.shape[0])), centroid)
        return self.apply(plan, img_u8_cuda, labels_u8_cuda) + (plan.scale_amt,)
