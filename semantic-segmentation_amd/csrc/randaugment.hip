// RandAugment on the device (datasets/randaugment.py: RandAugment.__call__ 256-263, augment_list 179-201,
// affine_transform 16-22; datasets/__init__.py:83-87 applies it under --rand_augment N,M to the cropped, mirrored
// (image, labels) pair, before ColorJitter): the drawn chain of up to SSA_RANDAUG_MAX_OPS of the 14 operations, every one
// bit-identical to the Pillow call the reference makes.  The draws stay on the host; what arrives here is the program
// (ssa_randaug_program: op codes, signed values, and for the five geometric operations the six affine coefficients the
// host prepared in fp64).  The arithmetic, as libImaging and ImageOps state it:
//   bilinear warp   (image under the shears and translations: transform(size, AFFINE, a, BILINEAR, fillcolor))  in fp64,
//                   left to right: xin = a0 (x + .5) + a1 (y + .5) + a2, yin likewise; outside [0, W) x [0, H) the fill;
//                   else both - .5, floor, dx, dy; columns x, x + 1 and row y clamped; v1 = p00 + (p01 - p00) dx; v2 the
//                   same on row y + 1 if that is inside, else v1; v = v1 + (v2 - v1) dy TRUNCATED.  No contraction.
//   nearest warp    (labels under the shears and Rotate, the image under Rotate: affine_fixed)  16.16 fixed point: the
//                   host fixes FIX(v) = floor(v 65536 + .5) of a0, a1, a3, a4 and of a2 + a0/2 + a1/2, a5 + a3/2 + a4/2;
//                   the source of (x, y) is ((f2 + y f1 + x f0) >> 16, (f5 + y f4 + x f3) >> 16) -- Pillow's integer
//                   recurrence in closed form --, copied if inside.
//   nearest, scale  (labels under the translations: a1 == a3 == 0 sends Pillow to ImagingScaleAffine)  a double that
//                   starts at a2 + .5 and grows by 1.0 per column, every sum rounded, truncated toward zero, negative =
//                   outside; rows likewise.  run_sum() gives the k-th partial sum without the scan.
//   AutoContrast    per band, lo / hi the first / last non-empty bin; hi <= lo: identity; else scale = 255.0 / (hi - lo),
//                   offset = -lo scale, lut[i] = clamp(int(i scale + offset)) in fp64, product and sum rounded apart.
//   Equalize        per band, integers: at most one non-empty bin: identity; step = (N - h[hi]) / 255, 0: identity; else
//                   lut[i] = min((step / 2 + sum_{j < i} h[j]) / step, 255) -- Image.point CLIPS entries above 255.
//   Invert 255 - i;  Solarize i < threshold ? i : 255 - i (float threshold);  Posterize i & ~(2^(8 - bits) - 1)
//   Color, Brightness   ImageEnhance.Color / Brightness: the blend of jitter_device.h against L of the pixel / black
//   Sharpness       blend(SMOOTH(img), img, v); SMOOTH = (1,1,1,1,5,1,1,1,1) / 13 + .5 truncated, border rows and
//                   columns copied.  Pillow sums in float32; s / 13 + .5 is never closer than 1/26 to an integer (2 s + 13
//                   is odd), so (2 s + 13) / 26 over the integer sum s is the same byte: the integer form is used.
// Kernels, all uint8 in and uint8 out, one launch per operation and buffer: a warp (image 3 channels, labels 1), a
// histogram of the window (3 x 256 counts, LDS atomics then one global atomic per non-empty bin and workgroup, into a
// buffer the caller zeroed), a point kernel (every per-pixel operation; for AutoContrast / Equalize each workgroup derives
// the 768-entry table from the histogram into LDS in its prologue: nothing is read back to the host), the Sharpness
// stencil on an LDS halo tile, and a crop / flip copy of image and labels for a chain that leaves one of them as it is.
// The first launch of a chain reads the source through the window and the flip; the later ones read what the one before
// wrote.  Byte streaming: 3 B (1 B) read and written per pixel and launch; the warps gather up to 4 source pixels.
#include "input_tail.h"

// Every product and sum below is rounded on its own, as the C code Pillow was compiled from rounds them (see gblur.hip).
#pragma clang fp contract(off)

namespace {

constexpr int TH = 16, TW = 64;                 // the Sharpness tile of the window
constexpr int SROW = (TW + 2) * 3;              // staged channel values per row
constexpr int NEAREST_MAX = 8192;               // the 16.16 sums stay inside Pillow's 32-bit ints up to this size

// A crop window of a uint8 [H][W][C] buffer, read mirrored under flip: (x, y) are window coordinates
struct Win {
  const unsigned char* p;
  int W, x0, y0, cw, ch, flip;
};

template <int C>
__device__ __forceinline__ const unsigned char* at(const Win& s, int x, int y) {
  return s.p + ((long)(s.y0 + y) * s.W + s.x0 + (s.flip ? s.cw - 1 - x : x)) * C;
}

__global__ __launch_bounds__(256) void copy_kernel(Win im, const unsigned char* __restrict__ lab,
                                                   unsigned char* __restrict__ img_out,
                                                   unsigned char* __restrict__ lab_out) {
  const long n = (long)im.cw * im.ch;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int y = (int)(i / im.cw), x = (int)(i - (long)y * im.cw);
    if (img_out) {
      const unsigned char* p = at<3>(im, x, y);
      unsigned char* o = img_out + i * 3;
      o[0] = p[0];
      o[1] = p[1];
      o[2] = p[2];
    }
    if (lab_out) {
      Win lw = im;
      lw.p = lab;
      lab_out[i] = *at<1>(lw, x, y);
    }
  }
}

// ------------------------------------------------------------------ warps
enum { WARP_BILINEAR = 0, WARP_FIXED = 1, WARP_SCALE = 2 };
struct WarpArg {
  double a[6];      // WARP_BILINEAR: the coefficients; WARP_SCALE: a[2], a[5] = the two starting sums
  long f[6];        // WARP_FIXED: the 16.16 coefficients
  int fill;
};

// The k-th partial sum of v + 1.0 + 1.0 + ... with every sum rounded to double, without the k additions: adding 1.0 is
// exact while the sum moves toward zero and while it stays inside one binade above 1; it rounds when it crosses 0, when it
// crosses 1 and at every power of two after that -- those steps are done as the single additions they are.
__device__ __forceinline__ double run_sum(double v, int k) {
  if (v <= -1.0) {
    double m = floor(-v);
    if (m > (double)k) m = (double)k;
    v += m;
    k -= (int)m;
  }
  while (k > 0 && v < 1.0) {
    v += 1.0;
    --k;
  }
  double top = 2.0;
  while (k > 0) {
    while (top <= v) top *= 2.0;
    const double room = ceil(top - v);            // the step that reaches or passes the next power of two
    if ((double)k < room) return v + (double)k;
    v = (v + (room - 1.0)) + 1.0;
    k -= (int)room;
  }
  return v;
}

__device__ __forceinline__ int coord(double v) { return v < 0.0 ? -1 : (int)v; }

template <int MODE, int C>
__global__ __launch_bounds__(256) void warp_kernel(Win s, WarpArg w, unsigned char* __restrict__ out) {
  const long n = (long)s.cw * s.ch;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int y = (int)(i / s.cw), x = (int)(i - (long)y * s.cw);
    unsigned char* o = out + i * C;
    if (MODE == WARP_BILINEAR) {
      const double xc = (double)x + 0.5, yc = (double)y + 0.5;
      double xin = w.a[0] * xc + w.a[1] * yc + w.a[2];
      double yin = w.a[3] * xc + w.a[4] * yc + w.a[5];
      if (!(xin >= 0.0 && xin < (double)s.cw && yin >= 0.0 && yin < (double)s.ch)) {
#pragma unroll
        for (int c = 0; c < C; ++c) o[c] = (unsigned char)w.fill;
        continue;
      }
      xin -= 0.5;
      yin -= 0.5;
      const double xf = floor(xin), yf = floor(yin);
      const double dx = xin - xf, dy = yin - yf;
      const int xi = (int)xf, yi = (int)yf;
      const int xa = min(max(xi, 0), s.cw - 1), xb = min(max(xi + 1, 0), s.cw - 1), ya = min(max(yi, 0), s.ch - 1);
      const bool below = yi + 1 >= 0 && yi + 1 < s.ch;
      const unsigned char *p00 = at<C>(s, xa, ya), *p01 = at<C>(s, xb, ya);
      const unsigned char *p10 = below ? at<C>(s, xa, yi + 1) : p00, *p11 = below ? at<C>(s, xb, yi + 1) : p01;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const double v1 = (double)p00[c] + ((double)p01[c] - (double)p00[c]) * dx;
        const double v2 = below ? (double)p10[c] + ((double)p11[c] - (double)p10[c]) * dx : v1;
        o[c] = (unsigned char)(int)(v1 + (v2 - v1) * dy);
      }
    } else {
      long xin, yin;
      if (MODE == WARP_FIXED) {
        xin = (w.f[2] + (long)y * w.f[1] + (long)x * w.f[0]) >> 16;
        yin = (w.f[5] + (long)y * w.f[4] + (long)x * w.f[3]) >> 16;
      } else {
        // the axis that is not translated starts at exactly 0.5: every partial sum k + 0.5 is exact
        xin = w.a[2] == 0.5 ? x : coord(run_sum(w.a[2], x));
        yin = w.a[5] == 0.5 ? y : coord(run_sum(w.a[5], y));
      }
      const bool inside = xin >= 0 && xin < s.cw && yin >= 0 && yin < s.ch;
      const unsigned char* p = inside ? at<C>(s, (int)xin, (int)yin) : nullptr;
#pragma unroll
      for (int c = 0; c < C; ++c) o[c] = inside ? p[c] : (unsigned char)w.fill;
    }
  }
}

// ------------------------------------------------------------------ histogram, tables, the point kernel
__global__ __launch_bounds__(256) void hist_kernel(Win s, unsigned int* __restrict__ hist) {
  __shared__ unsigned int h[768];
  for (int k = threadIdx.x; k < 768; k += 256) h[k] = 0;
  __syncthreads();
  const long n = (long)s.cw * s.ch, stride = (long)gridDim.x * blockDim.x;
  // four pixels per step: their twelve loads are issued before the first LDS atomic
  for (long i0 = blockIdx.x * (long)blockDim.x + threadIdx.x; i0 < n; i0 += 4 * stride) {
    int v[4][3];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long i = i0 + u * stride;
      v[u][0] = -1;
      if (i < n) {
        const int y = (int)(i / s.cw), x = (int)(i - (long)y * s.cw);
        const unsigned char* p = at<3>(s, x, y);
        v[u][0] = p[0];
        v[u][1] = p[1];
        v[u][2] = p[2];
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (v[u][0] >= 0) {
        atomicAdd(&h[v[u][0]], 1u);
        atomicAdd(&h[256 + v[u][1]], 1u);
        atomicAdd(&h[512 + v[u][2]], 1u);
      }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < 768; k += 256)
    if (h[k]) atomicAdd(&hist[k], h[k]);
}

struct PointArg {
  int op;            // SSA_RANDAUG_*
  int mask;          // Posterize
  float f;           // Color, Brightness
  double threshold;  // Solarize
};

// The 768-entry table of AutoContrast / Equalize from the window's histogram (n pixels), entry tid of every band
__device__ __forceinline__ void build_lut(int op, const unsigned int* __restrict__ hist, long n, unsigned char* lut) {
  __shared__ unsigned int h[768];
  __shared__ unsigned int pre[2][768];            // Equalize: the running sums of h, doubling the reach per step
  __shared__ int part[4][9];                      // per wave and band: first and last non-empty bin, their number
  __shared__ int lo[3], hi[3], filled[3];
  const int tid = threadIdx.x;
  for (int c = 0; c < 3; ++c) h[c * 256 + tid] = pre[0][c * 256 + tid] = hist[c * 256 + tid];
  __syncthreads();
  // reduced by shuffles and once through LDS: 256 LDS atomics on one word would be served one lane at a time
  for (int c = 0; c < 3; ++c) {
    const bool any = h[c * 256 + tid] != 0;
    int l = any ? tid : 256, u = any ? tid : -1, f = any ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      l = min(l, __shfl_xor(l, o, 64));
      u = max(u, __shfl_xor(u, o, 64));
      f += __shfl_xor(f, o, 64);
    }
    if ((tid & 63) == 0) {
      part[tid >> 6][c] = l;
      part[tid >> 6][3 + c] = u;
      part[tid >> 6][6 + c] = f;
    }
  }
  __syncthreads();
  if (tid < 3) {
    lo[tid] = min(min(part[0][tid], part[1][tid]), min(part[2][tid], part[3][tid]));
    hi[tid] = max(max(part[0][3 + tid], part[1][3 + tid]), max(part[2][3 + tid], part[3][3 + tid]));
    filled[tid] = part[0][6 + tid] + part[1][6 + tid] + part[2][6 + tid] + part[3][6 + tid];
  }
  __syncthreads();
  int b = 0;
  if (op == SSA_RANDAUG_EQUALIZE)
    for (int d = 1; d < 256; d <<= 1, b ^= 1) {
      for (int c = 0; c < 3; ++c)
        pre[b ^ 1][c * 256 + tid] = pre[b][c * 256 + tid] + (tid >= d ? pre[b][c * 256 + tid - d] : 0u);
      __syncthreads();
    }
  for (int c = 0; c < 3; ++c) {
    int v = tid;
    if (op == SSA_RANDAUG_AUTOCONTRAST) {
      if (hi[c] > lo[c]) {
        const double scale = 255.0 / (double)(hi[c] - lo[c]);
        const double offset = -(double)lo[c] * scale;
        const double t = (double)tid * scale + offset;
        v = t <= 0.0 ? 0 : (t >= 255.0 ? 255 : (int)t);    // int() of a value in (-1, 0) is 0 as well
      }
    } else if (filled[c] > 1) {
      // n < 2^31 (checked by the entry point): step / 2 + the bins below tid stays inside 32 bits
      const unsigned int step = ((unsigned int)n - h[c * 256 + hi[c]]) / 255u;
      if (step) {
        const unsigned int q = (step / 2 + (pre[b][c * 256 + tid] - h[c * 256 + tid])) / step;
        v = q > 255u ? 255 : (int)q;
      }
    }
    lut[c * 256 + tid] = (unsigned char)v;
  }
  __syncthreads();
}

__global__ __launch_bounds__(256) void point_kernel(Win s, PointArg a, const unsigned int* __restrict__ hist,
                                                    unsigned char* __restrict__ out) {
  __shared__ unsigned char lut[768];
  const long n = (long)s.cw * s.ch;
  const bool table = a.op == SSA_RANDAUG_AUTOCONTRAST || a.op == SSA_RANDAUG_EQUALIZE;
  if (table) build_lut(a.op, hist, n, lut);
  const bool clip = blend_clips(a.f);
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int y = (int)(i / s.cw), x = (int)(i - (long)y * s.cw);
    const unsigned char* p = at<3>(s, x, y);
    int c3[3] = {p[0], p[1], p[2]};
    if (table) {
#pragma unroll
      for (int c = 0; c < 3; ++c) c3[c] = lut[c * 256 + c3[c]];
    } else if (a.op == SSA_RANDAUG_INVERT) {
#pragma unroll
      for (int c = 0; c < 3; ++c) c3[c] = 255 - c3[c];
    } else if (a.op == SSA_RANDAUG_SOLARIZE) {
#pragma unroll
      for (int c = 0; c < 3; ++c) c3[c] = (double)c3[c] < a.threshold ? c3[c] : 255 - c3[c];
    } else if (a.op == SSA_RANDAUG_POSTERIZE) {
#pragma unroll
      for (int c = 0; c < 3; ++c) c3[c] &= a.mask;
    } else {                                      // Color: against L of the pixel; Brightness: against black
      const int d = a.op == SSA_RANDAUG_COLOR ? luma(c3[0], c3[1], c3[2]) : 0;
#pragma unroll
      for (int c = 0; c < 3; ++c) c3[c] = blend(d, c3[c], a.f, clip);
    }
    unsigned char* o = out + i * 3;
    o[0] = (unsigned char)c3[0];
    o[1] = (unsigned char)c3[1];
    o[2] = (unsigned char)c3[2];
  }
}

// ------------------------------------------------------------------ Sharpness
// A workgroup of 256 owns a TH x TW tile of the window: it stages the tile and a halo of one pixel (clamped to the window;
// the clamped values are never used, the window's border is copied) and blends SMOOTH with the pixel.
__global__ __launch_bounds__(256) void sharpness_kernel(Win s, float f, unsigned char* __restrict__ out) {
  __shared__ unsigned char px[(TH + 2) * SROW];
  const int tid = threadIdx.x;
  const int tx = blockIdx.x * TW, ty = blockIdx.y * TH;
  for (int i = tid; i < (TH + 2) * (TW + 2); i += 256) {
    const int hy = i / (TW + 2), hx = i - hy * (TW + 2);
    const int oy = min(max(ty + hy - 1, 0), s.ch - 1), ox = min(max(tx + hx - 1, 0), s.cw - 1);
    const unsigned char* p = at<3>(s, ox, oy);
    unsigned char* q = px + hy * SROW + hx * 3;
    q[0] = p[0];
    q[1] = p[1];
    q[2] = p[2];
  }
  __syncthreads();
  const bool clip = blend_clips(f);
  for (int i = tid; i < TH * TW * 3; i += 256) {
    const int r = i / (TW * 3), k = i - r * (TW * 3);
    const int y = ty + r, x = tx + k / 3;
    if (y >= s.ch || x >= s.cw) continue;
    const unsigned char* q = px + (r + 1) * SROW + 3 + k;
    int v = q[0];
    if (y > 0 && y < s.ch - 1 && x > 0 && x < s.cw - 1) {
      const int sum = q[-SROW - 3] + q[-SROW] + q[-SROW + 3] + q[-3] + 5 * v + q[3] + q[SROW - 3] + q[SROW] + q[SROW + 3];
      v = blend((2 * sum + 13) / 26, v, f, clip);
    }
    out[((long)y * s.cw + x) * 3 + k % 3] = (unsigned char)v;
  }
}

bool geometric(int op) { return op >= SSA_RANDAUG_SHEARX && op <= SSA_RANDAUG_ROTATE; }

// An operation that leaves the pair as it is: Identity, and Rotate by a multiple of 360 degrees (Image.rotate copies)
bool is_copy(int op, double value) {
  return op == SSA_RANDAUG_IDENTITY || (op == SSA_RANDAUG_ROTATE && std::fmod(value, 360.0) == 0.0);
}

long fix16(double v) { return (long)std::floor(v * 65536.0 + 0.5); }

}  // namespace

extern "C" {

int ssa_randaug_u8(const unsigned char* img_hwc, const unsigned char* lab_hw, int H, int W, int x0, int y0, int cw,
                   int ch, int flip, const ssa_randaug_program* program, int ignore_label, unsigned int* hist,
                   unsigned char* img_out, unsigned char* img_tmp, unsigned char* lab_out, unsigned char* lab_tmp,
                   void* stream) {
  if (!img_hwc || !img_out || !program || !window_ok(H, W, x0, y0, cw, ch)) return SSA_EINVAL;
  if (lab_hw && !lab_out) return SSA_EINVAL;
  if (ignore_label < 0 || ignore_label > 255) return SSA_EINVAL;
  if (program->n_ops < 0 || program->n_ops > SSA_RANDAUG_MAX_OPS) return SSA_EINVAL;
  int n_img = 0, n_lab = 0, n_hist = 0;
  bool nearest = false;
  for (int k = 0; k < program->n_ops; ++k) {
    const int op = program->op[k];
    const double v = program->value[k];
    if (op < 0 || op >= SSA_RANDAUG_N_OPS || !std::isfinite(v)) return SSA_EINVAL;
    if (op == SSA_RANDAUG_POSTERIZE && !(v == 4.0 || v == 5.0 || v == 6.0 || v == 7.0 || v == 8.0)) return SSA_EINVAL;
    if (is_copy(op, v)) continue;
    ++n_img;
    if (geometric(op)) {
      for (int j = 0; j < 6; ++j)
        if (!std::isfinite(program->matrix[k][j])) return SSA_EINVAL;
      const double* a = program->matrix[k];
      const bool scale = a[1] == 0.0 && a[3] == 0.0;
      if (scale && (a[0] != 1.0 || a[4] != 1.0)) return SSA_EUNSUPPORTED;   // only the translations take that routine
      if (lab_hw) {
        ++n_lab;
        nearest = nearest || !scale;
      }
      nearest = nearest || op == SSA_RANDAUG_ROTATE;
    }
    if (op == SSA_RANDAUG_AUTOCONTRAST || op == SSA_RANDAUG_EQUALIZE) ++n_hist;
  }
  if (n_img > 1 && !img_tmp) return SSA_EINVAL;
  if (n_lab > 1 && !lab_tmp) return SSA_EINVAL;
  if (n_hist && (!hist || (reinterpret_cast<uintptr_t>(hist) & 3u) || (long)cw * ch > 0x7fffffffL)) return SSA_EINVAL;
  if ((ch + TH - 1) / TH > 65535) return SSA_EINVAL;
  if (nearest && (cw > NEAREST_MAX || ch > NEAREST_MAX)) return SSA_EUNSUPPORTED;

  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(stream_blocks((long)cw * ch)), block(256);
  const int fl = flip ? 1 : 0;
  // the k-th of n launches writes `out` when an even number of launches follow it: the last one always does
  Win im{img_hwc, W, x0, y0, cw, ch, fl}, lb{lab_hw, W, x0, y0, cw, ch, fl};
  int i_img = 0, i_lab = 0, i_hist = 0;
  if (n_img == 0 || (lab_hw && n_lab == 0)) {      // what no operation rewrites is copied through the window, once
    hipLaunchKernelGGL(copy_kernel, grid, block, 0, st, im, lab_hw, n_img == 0 ? img_out : (unsigned char*)nullptr,
                       (lab_hw && n_lab == 0) ? lab_out : (unsigned char*)nullptr);
    SSA_LAUNCH_CHECK();
  }
  for (int k = 0; k < program->n_ops; ++k) {
    const int op = program->op[k];
    const double v = program->value[k];
    if (is_copy(op, v)) continue;
    unsigned char* dst = (n_img - 1 - i_img) % 2 == 0 ? img_out : img_tmp;
    if (geometric(op)) {
      const double* a = program->matrix[k];
      WarpArg w{};
      for (int j = 0; j < 6; ++j) w.a[j] = a[j];
      w.f[0] = fix16(a[0]);
      w.f[1] = fix16(a[1]);
      w.f[2] = fix16(a[2] + a[0] * 0.5 + a[1] * 0.5);
      w.f[3] = fix16(a[3]);
      w.f[4] = fix16(a[4]);
      w.f[5] = fix16(a[5] + a[3] * 0.5 + a[4] * 0.5);
      w.fill = 0;
      if (op == SSA_RANDAUG_ROTATE)
        hipLaunchKernelGGL((warp_kernel<WARP_FIXED, 3>), grid, block, 0, st, im, w, dst);
      else
        hipLaunchKernelGGL((warp_kernel<WARP_BILINEAR, 3>), grid, block, 0, st, im, w, dst);
      SSA_LAUNCH_CHECK();
      if (lab_hw) {
        unsigned char* ldst = (n_lab - 1 - i_lab) % 2 == 0 ? lab_out : lab_tmp;
        w.fill = ignore_label;
        if (a[1] == 0.0 && a[3] == 0.0) {
          w.a[2] = a[2] + a[0] * 0.5;
          w.a[5] = a[5] + a[4] * 0.5;
          hipLaunchKernelGGL((warp_kernel<WARP_SCALE, 1>), grid, block, 0, st, lb, w, ldst);
        } else {
          hipLaunchKernelGGL((warp_kernel<WARP_FIXED, 1>), grid, block, 0, st, lb, w, ldst);
        }
        SSA_LAUNCH_CHECK();
        lb = Win{ldst, cw, 0, 0, cw, ch, 0};
        ++i_lab;
      }
    } else if (op == SSA_RANDAUG_SHARPNESS) {
      hipLaunchKernelGGL(sharpness_kernel, dim3((cw + TW - 1) / TW, (ch + TH - 1) / TH), block, 0, st, im, (float)v, dst);
      SSA_LAUNCH_CHECK();
    } else {
      PointArg pa{op, 0, 1.f, 0.0};
      const unsigned int* h = nullptr;
      if (op == SSA_RANDAUG_AUTOCONTRAST || op == SSA_RANDAUG_EQUALIZE) {
        unsigned int* hk = hist + 768 * i_hist++;
        // one workgroup per CU at most: each one ends with up to 768 global atomics
        hipLaunchKernelGGL(hist_kernel, dim3(grid.x < 256 ? grid.x : 256), block, 0, st, im, hk);
        SSA_LAUNCH_CHECK();
        h = hk;
      } else if (op == SSA_RANDAUG_SOLARIZE) {
        pa.threshold = v;
      } else if (op == SSA_RANDAUG_POSTERIZE) {
        pa.mask = ~((1 << (8 - (int)v)) - 1) & 255;
      } else if (op != SSA_RANDAUG_INVERT) {
        pa.f = (float)v;
      }
      // every workgroup of a table operation pays the table's prologue: a quarter of the streaming grid
      hipLaunchKernelGGL(point_kernel, dim3(h && grid.x > 1024 ? 1024 : grid.x), block, 0, st, im, pa, h, dst);
      SSA_LAUNCH_CHECK();
    }
    im = Win{dst, cw, 0, 0, cw, ch, 0};
    ++i_img;
  }
  return SSA_OK;
}

}  // extern "C"
