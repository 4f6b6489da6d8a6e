// RandomGaussianBlur on the device (transforms/transforms.py:154-162, datasets/__init__.py:102 under --gblur): the
// image-only augmentation the reference's loader runs after ColorJitter and before ToTensor + Normalize --
//   blurred = skimage.filters.gaussian(np.array(img), sigma, multichannel=True); blurred *= 255; .astype(uint8)
// with sigma = 0.15 + random.random() * 1.15 drawn on the host.  skimage's function converts the bytes to float64
// (x * (1 / 255), the 256-entry table `lut256` the host uploads) and calls scipy.ndimage.gaussian_filter(image,
// [sigma, sigma, 0], mode='nearest', truncate=4.0): two passes of SciPy's correlate1d in its symmetric branch, the
// vertical one first, each over an image whose indices are clamped to its edges.  With r = int(4 sigma + 0.5) in 1..5
// and the normalised weights w[0..r] (w[j] at distance j; the host derives them as _gaussian_kernel1d does) one pass is
//   t = x[i] * w[0];   for j = r, r - 1, ..., 1:   t += (x[i - j] + x[i + j]) * w[j]
// in float64, every sum and every product rounded on its own; the result is t * 255.0 truncated toward zero to a byte.
// The truncation makes the last bit matter: the weights sum to 1 +- 1 ulp, so of 768 constant images (256 grey levels,
// sigma 0.3, 0.7, 1.1) 308 leave the reference one grey level darker, and a fused multiply-add or another order of the
// sum moves such pixels.  Hence fp64 in exactly this order and no contraction (see the pragma below).
//
// One kernel, two stores.  A workgroup of 256 owns a 16 x 64 tile of the window: it stages the bytes of the tile and of
// a halo of r pixels on every side into LDS -- coordinates clamped to the CROP WINDOW (the reference blurs the cropped
// image), the horizontal flip applied at the load, and the ColorJitter program, where one is given, run on every staged
// pixel with the contrast mean read from the counter ssa_jitter_luma_sum left (no host synchronisation) --, runs the
// vertical pass into fp64 LDS over the tile's columns plus the horizontal halo, the horizontal pass from there, and
// stores either the bytes (ssa_gblur_u8) or what ssa_image_u8_crop_flip_normalize makes of them
// (ssa_gblur_crop_flip_normalize).  Per pixel 3 B read (halo overlap served by L2) and 3 B or 32 B written; 39 KB of
// static LDS.
#include "input_tail.h"

// Every product and sum below is rounded on its own, as the C code SciPy was compiled from rounds them: hipcc
// contracts a * b + c to one v_fma_f64 by default, across statements and through inlined functions.
#pragma clang fp contract(off)

namespace {

constexpr int TH = 16, TW = 64, RMAX = 5;       // tile of the window, largest radius
constexpr int HH = TH + 2 * RMAX;               // staged rows
constexpr int HROW = (TW + 2 * RMAX) * 3;       // staged channel values per row (222)

// One pass at one position: x(0) loads the centre, x(-j * stride) and x(j * stride) the pair at distance j
template <typename Load>
__device__ __forceinline__ double blur_pass(const ssa_gblur_taps& tp, Load x, int stride) {
#pragma clang fp contract(off)
  double t = x(0) * tp.w[0];
#pragma unroll
  for (int j = RMAX; j >= 1; --j)
    if (j <= tp.radius) t += (x(-j * stride) + x(j * stride)) * tp.w[j];
  return t;
}

template <bool NORM>
__global__ __launch_bounds__(256) void gblur_kernel(const unsigned char* __restrict__ img, int W, int x0, int y0,
                                                    int cw, int ch, int flip, ssa_jitter_program pg,
                                                    const unsigned long long* __restrict__ counter,
                                                    ssa_gblur_taps tp, const double* __restrict__ lut, Norm3 nm,
                                                    void* __restrict__ out, int cpad) {
  __shared__ double s_lut[256];
  __shared__ double s_v[TH * HROW];             // the vertical pass: tile rows x (tile + halo) columns x 3
  __shared__ unsigned char s_px[HH * HROW];     // the staged bytes
  __shared__ unsigned char s_out[TH * TW * 3];  // the blurred bytes of the tile
  const int tid = threadIdx.x, R = tp.radius;
  const int tx = blockIdx.x * TW, ty = blockIdx.y * TH;
  const int hw = TW + 2 * R, hh = TH + 2 * R;
  const int m = contrast_mean(pg, counter, (long)cw * ch);
  s_lut[tid] = lut[tid];
  for (int i = tid; i < hh * hw; i += 256) {
    const int hy = i / hw, hx = i - hy * hw;
    const int oy = min(max(ty + hy - R, 0), ch - 1), ox = min(max(tx + hx - R, 0), cw - 1);
    const unsigned char* p = img + ((long)(y0 + oy) * W + x0 + (flip ? cw - 1 - ox : ox)) * 3;
    int r = p[0], g = p[1], b = p[2];
    jitter_pixel(pg, m, r, g, b);
    unsigned char* s = s_px + hy * HROW + hx * 3;
    s[0] = (unsigned char)r;
    s[1] = (unsigned char)g;
    s[2] = (unsigned char)b;
  }
  __syncthreads();
  const int rowlen = hw * 3;
  for (int i = tid; i < TH * rowlen; i += 256) {
    const int r = i / rowlen, k = i - r * rowlen;
    const unsigned char* p = s_px + (r + R) * HROW + k;
    s_v[r * HROW + k] = blur_pass(tp, [&](int o) { return s_lut[p[o]]; }, HROW);
  }
  __syncthreads();
  for (int i = tid; i < TH * TW * 3; i += 256) {
    const int r = i / (TW * 3), k = i - r * (TW * 3);
    const double* q = s_v + r * HROW + R * 3 + k;
    const double t = blur_pass(tp, [&](int o) { return q[o]; }, 3);
    s_out[i] = (unsigned char)(int)(t * 255.0);
  }
  __syncthreads();
  if (!NORM) {
    unsigned char* o = (unsigned char*)out;
    for (int i = tid; i < TH * TW * 3; i += 256) {
      const int r = i / (TW * 3), k = i - r * (TW * 3);
      const int y = ty + r;
      const long xb = (long)tx * 3 + k;
      if (y < ch && xb < (long)cw * 3) o[(long)y * cw * 3 + xb] = s_out[i];
    }
  } else {
    for (int i = tid; i < TH * TW; i += 256) {
      const int r = i / TW, x = i - r * TW;
      if (ty + r >= ch || tx + x >= cw) continue;
      const unsigned char* p = s_out + i * 3;
      store_normalized(p[0], p[1], p[2], nm, (bf16_t*)out + ((long)(ty + r) * cw + tx + x) * cpad, cpad);
    }
  }
}

// Everything both entry points check; fills the program the kernel takes (none: zero steps)
bool gblur_args_ok(const unsigned char* img, int H, int W, int x0, int y0, int cw, int ch,
                   const ssa_jitter_program* program, const unsigned long long* counter, const ssa_gblur_taps* taps,
                   const double* lut256, const void* out, ssa_jitter_program* pg) {
  if (!img || !out || !taps || !lut256 || (reinterpret_cast<uintptr_t>(lut256) & 7u)) return false;
  if (!window_ok(H, W, x0, y0, cw, ch) || (ch + TH - 1) / TH > 65535) return false;
  if (taps->radius < 1 || taps->radius > RMAX) return false;
  for (int j = 0; j <= RMAX; ++j)
    if (!std::isfinite(taps->w[j])) return false;
  *pg = ssa_jitter_program{};
  if (program) {
    bool contrast = false;
    if (!program_ok(program, &contrast)) return false;
    if (contrast && (!counter || (reinterpret_cast<uintptr_t>(counter) & 7u))) return false;
    *pg = *program;
  }
  return true;
}

dim3 gblur_grid(int cw, int ch) { return dim3((cw + TW - 1) / TW, (ch + TH - 1) / TH); }

}  // namespace

extern "C" {

int ssa_gblur_u8(const unsigned char* img_hwc, int H, int W, int x0, int y0, int cw, int ch, int flip,
                 const ssa_jitter_program* program, const unsigned long long* counter, const ssa_gblur_taps* taps,
                 const double* lut256, unsigned char* out_hwc, void* stream) {
  ssa_jitter_program pg;
  if (!gblur_args_ok(img_hwc, H, W, x0, y0, cw, ch, program, counter, taps, lut256, out_hwc, &pg)) return SSA_EINVAL;
  hipLaunchKernelGGL(gblur_kernel<false>, gblur_grid(cw, ch), dim3(256), 0, (hipStream_t)stream, img_hwc, W, x0, y0,
                     cw, ch, flip ? 1 : 0, pg, counter, *taps, lut256, Norm3{}, (void*)out_hwc, 0);
  SSA_LAUNCH_CHECK();
  return SSA_OK;
}

int ssa_gblur_crop_flip_normalize(const unsigned char* img_hwc, int H, int W, int x0, int y0, int cw, int ch,
                                  int flip, const ssa_jitter_program* program, const unsigned long long* counter,
                                  const ssa_gblur_taps* taps, const double* lut256, const float* mean3,
                                  const float* std3, void* out_nhwc, int cpad, void* stream) {
  ssa_jitter_program pg;
  Norm3 nm;
  if (!gblur_args_ok(img_hwc, H, W, x0, y0, cw, ch, program, counter, taps, lut256, out_nhwc, &pg) || cpad != 16 ||
      !norm3_ok(mean3, std3, out_nhwc, cpad, &nm))
    return SSA_EINVAL;
  hipLaunchKernelGGL(gblur_kernel<true>, gblur_grid(cw, ch), dim3(256), 0, (hipStream_t)stream, img_hwc, W, x0, y0,
                     cw, ch, flip ? 1 : 0, pg, counter, *taps, lut256, nm, out_nhwc, cpad);
  SSA_LAUNCH_CHECK();
  return SSA_OK;
}

}  // extern "C"
