"""NumPy restatement of the reference's RandomGaussianBlur (transforms/transforms.py:154-162):

    blurred = skimage.filters.gaussian(np.array(img), sigma=sigma, multichannel=True);  blurred *= 255;  .astype(np.uint8)

skimage's function converts the bytes to float64 (`to_float64`, the wrapper assumption: np.multiply(image, 1 / 255,
dtype=float64) of skimage/util/dtype.py) and calls scipy.ndimage.gaussian_filter(image, [sigma, sigma, 0], mode='nearest',
truncate=4.0): correlate1d along axis 0, then along axis 1, in the symmetric branch of ni_filters.c --
    t = x[i] * w[0];   for j = r ... 1:   t += (x[i - j] + x[i + j]) * w[j]
with the indices clamped to the image.  NumPy evaluates each of these operations on its own (no contraction), in float64.
tests/test_gblur_cpu.py pins this file to live SciPy, to scikit-image wherever it is installed, and to the fixture recorded
from the reference; the device tests compare the kernels with it.  Nothing here imports the code under test."""
import json
import os

import numpy as np


def to_float64(img_u8):
    """What skimage's img_as_float makes of a uint8 image."""
    return np.multiply(img_u8, 1 / 255, dtype=np.float64)


def taps(sigma):
    """(radius, weights at distance 0..radius) of scipy.ndimage.gaussian_filter1d at truncate=4.0."""
    sigma = float(sigma)
    radius = int(4.0 * sigma + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    return radius, phi[radius:]


def correlate_axis(x, w, axis):
    """One pass of the symmetric correlate1d with mode='nearest' along `axis` (w: weights at distance 0..r)."""
    n, r = x.shape[axis], len(w) - 1
    idx = np.arange(n)
    t = x * w[0]
    for j in range(r, 0, -1):
        lo = np.take(x, np.clip(idx - j, 0, n - 1), axis=axis)
        hi = np.take(x, np.clip(idx + j, 0, n - 1), axis=axis)
        t = t + (lo + hi) * w[j]
    return t


def blur_float(img_u8, sigma):
    """float64 [h, w, 3]: gaussian(img, sigma, multichannel=True)."""
    _, w = taps(sigma)
    return correlate_axis(correlate_axis(to_float64(img_u8), w, 0), w, 1)


def blur(img_u8, sigma, window=None, flip=False):
    """The blur of the crop window (x0, y0, w, h) of img_u8, mirrored first when flip is set (the reference crops and
    flips before its image-only transforms) -> uint8."""
    if window is not None:
        x0, y0, w, h = window
        img_u8 = img_u8[y0:y0 + h, x0:x0 + w]
    if flip:
        img_u8 = img_u8[:, ::-1]
    out = blur_float(np.ascontiguousarray(img_u8), sigma)
    out *= 255
    return out.astype(np.uint8)


def levels_image():
    """256 x 256 x 3: 16 x 16 blocks of 16 x 16 pixels, block k constant at grey level k.  At radius 5 the 6 x 6 interior of
    every block sees a constant neighbourhood: there the result is level * (1 / 255) * (sum of the weights as the pass
    adds them), twice, times 255 -- within an ulp or two of an integer, where the last bit decides the byte."""
    k = np.arange(256, dtype=np.uint8).reshape(16, 16)
    return np.ascontiguousarray(np.repeat(np.repeat(k, 16, 0), 16, 1)[..., None].repeat(3, -1))


def load_golden():
    """tests/golden/gblur_golden.npz (make_golden_gblur.py) -> (inputs [list of uint8 h x w x 3], outputs [same], meta)."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gblur_golden.npz"))
    meta = json.loads(str(z["meta"]))
    n = len(meta["entries"])
    return [z["in%d" % i] for i in range(n)], [z["out%d" % i] for i in range(n)], meta
