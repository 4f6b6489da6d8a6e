// ColorJitter on the device (transforms/transforms.py:192-362, datasets/__init__.py:94-99): the image-only
// augmentation the reference's loader runs between the joint crop / flip and ToTensor + Normalize --
// ImageEnhance.Brightness / Contrast / Color and the HSV round trip of adjust_hue, in the shuffled order that
// ColorJitter.get_params drew.  Every step is defined on bytes, so the kernels reproduce Pillow bit for bit:
//   luma     L = (R*19595 + G*38470 + B*7471 + 0x8000) >> 16                        (convert("L"))
//   blend    t = fp32(d) + f * (fp32(x) - fp32(d)), multiply and add rounded separately (Image.blend); truncated
//            for 0 <= f <= 1, clipped to [0, 255] and truncated otherwise.  d = 0 (brightness), d = L of the pixel
//            (saturation), d = m = int(sum(L) / N + 0.5) over the image as it is when contrast runs (contrast)
//   hue      RGB -> HSV (fp32 with the two double detours of libImaging/Convert.c), H += byte mod 256, HSV -> RGB
// A jitter PROGRAM (ssa_jitter_program: up to four op codes in application order, three factors, the hue byte)
// travels by value as a kernel argument.  The contrast mean needs the whole window first: jitter_luma_sum_kernel
// applies the steps that precede contrast in registers and adds L into one 64-bit counter (integer sums: exact
// and order-independent); the apply kernels read that counter on the device and form m themselves, so the pair
// needs no host synchronisation and can be captured into a graph.
// Byte streaming, HBM-bound: 3 B read per pixel per kernel; 3 B (uint8) or 32 B (normalised NHWC, 16-channel
// padded, the trunk's input) written.
#include "common.h"
#include "../../include/semseg_hip.h"

// Every product and sum in this file is rounded on its own, as the C code Pillow was compiled from rounds them: no
// contraction to FMA.  hipcc contracts by default, across statements and through inlined functions, and the
// __fmul_rn / __fadd_rn of the HIP headers do not stop it: they are inline functions over the plain operators, compiled
// under the default, so d + f * (x - d) written with them still came out as one v_fma_f32 (0.8 * -145 + 147 = 30.999998
// instead of 31).  Hence plain operators under this pragma for every multiply, add and subtract below.
#pragma clang fp contract(off)

namespace {

struct Norm3 { float mean[3], stdv[3]; };

__device__ __forceinline__ int luma(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

// Image.blend(degenerate, img, f) of one channel
__device__ __forceinline__ int blend(int d, int x, float f, bool clip) {
#pragma clang fp contract(off)
  const float t = (float)d + f * ((float)x - (float)d);
  if (clip) {
    if (t <= 0.f) return 0;
    if (t >= 255.f) return 255;
  }
  return (int)t;
}

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// rgb2hsv + (H + shift) mod 256 + hsv2rgb of libImaging/Convert.c
__device__ __forceinline__ void hue_shift(int& r, int& g, int& b, int shift) {
#pragma clang fp contract(off)
  const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
  if (maxc == minc) return;                       // S == 0: grey V whatever H is
  const float cr = (float)(maxc - minc);
  const float s = __fdiv_rn(cr, (float)maxc);
  const float rc = __fdiv_rn((float)(maxc - r), cr), gc = __fdiv_rn((float)(maxc - g), cr),
              bc = __fdiv_rn((float)(maxc - b), cr);
  float h;
  if (r == maxc) h = bc - gc;
  else if (g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
  else h = (float)(4.0 + (double)gc - (double)rc);
  double hd = (double)h / 6.0 + 1.0;              // in [5/6, 11/6]; fmod(hd, 1.0) is this exact subtraction
  if (hd >= 1.0) hd -= 1.0;
  h = (float)hd;
  const int H = (clip8((int)((double)h * 255.0)) + shift) & 255;
  const int S = clip8((int)((double)s * 255.0)), V = maxc;
  if (S == 0) { r = g = b = V; return; }
  const double hf = (double)H * 6.0 / 255.0;
  const int i = (int)floor(hf);
  const double f = hf - (double)i, fs = (double)S / 255.0, v = (double)V;
  const int p = clip8((int)floor(v * (1.0 - fs) + 0.5));
  const int q = clip8((int)floor(v * (1.0 - fs * f) + 0.5));
  const int t = clip8((int)floor(v * (1.0 - fs * (1.0 - f)) + 0.5));
  switch (i % 6) {
    case 0: r = V; g = t; b = p; break;
    case 1: r = q; g = V; b = p; break;
    case 2: r = p; g = V; b = t; break;
    case 3: r = p; g = q; b = V; break;
    case 4: r = t; g = p; b = V; break;
    default: r = V; g = p; b = q; break;
  }
}

__device__ __forceinline__ bool blend_clips(float f) { return !(f >= 0.f && f <= 1.f); }

// One step of the program on one pixel (m: the contrast mean; unused by the other steps)
__device__ __forceinline__ void jitter_step(const ssa_jitter_program& pg, int op, int m, int& r, int& g, int& b) {
  if (op == SSA_JITTER_HUE) {
    hue_shift(r, g, b, pg.hue_byte);
    return;
  }
  const float f = pg.factor[op];
  const bool clip = blend_clips(f);
  if (op == SSA_JITTER_SATURATION) m = luma(r, g, b);
  else if (op == SSA_JITTER_BRIGHTNESS) m = 0;
  r = blend(m, r, f, clip);
  g = blend(m, g, f, clip);
  b = blend(m, b, f, clip);
}

// The steps in front of the (first) contrast step, then L: what ImageEnhance.Contrast averages
__device__ __forceinline__ int jitter_luma_before_contrast(const ssa_jitter_program& pg, int r, int g, int b) {
  for (int k = 0; k < pg.n_ops && pg.op[k] != SSA_JITTER_CONTRAST; ++k) jitter_step(pg, pg.op[k], 0, r, g, b);
  return luma(r, g, b);
}

__device__ __forceinline__ void jitter_pixel(const ssa_jitter_program& pg, int m, int& r, int& g, int& b) {
  for (int k = 0; k < pg.n_ops; ++k) jitter_step(pg, pg.op[k], m, r, g, b);
}

// m = int(S / N + 0.5) with the division in double (ImageStat.Stat(...).mean[0] + 0.5, truncated)
__device__ __forceinline__ int contrast_mean(const ssa_jitter_program& pg, const unsigned long long* counter, long n) {
  for (int k = 0; k < pg.n_ops; ++k)
    if (pg.op[k] == SSA_JITTER_CONTRAST) return (int)((double)*counter / (double)n + 0.5);
  return 0;
}

// Zeroes the counter in stream order, as a kernel node of its own: captured into a graph with the luma sum and the apply,
// it clears the word at the start of every replay.
__global__ void jitter_clear_kernel(unsigned long long* __restrict__ counter) { *counter = 0; }

__global__ __launch_bounds__(256) void jitter_luma_sum_kernel(const unsigned char* __restrict__ img, int W, int x0,
                                                              int y0, int cw, int ch, ssa_jitter_program pg,
                                                              unsigned long long* __restrict__ counter) {
  __shared__ unsigned long long red[4];
  const long n = (long)cw * ch;
  unsigned long long acc = 0;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int y = (int)(i / cw), x = (int)(i - (long)y * cw);
    const unsigned char* p = img + ((long)(y0 + y) * W + x0 + x) * 3;
    acc += (unsigned long long)jitter_luma_before_contrast(pg, p[0], p[1], p[2]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(counter, red[0] + red[1] + red[2] + red[3]);
}

__global__ __launch_bounds__(256) void jitter_apply_u8_kernel(const unsigned char* __restrict__ img, int W, int x0,
                                                              int y0, int cw, int ch, int flip, ssa_jitter_program pg,
                                                              const unsigned long long* __restrict__ counter,
                                                              unsigned char* __restrict__ out) {
  const long n = (long)cw * ch;
  const int m = contrast_mean(pg, counter, n);
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int y = (int)(i / cw), x = (int)(i - (long)y * cw);
    const int sx = x0 + (flip ? cw - 1 - x : x), sy = y0 + y;
    const unsigned char* p = img + ((long)sy * W + sx) * 3;
    int r = p[0], g = p[1], b = p[2];
    jitter_pixel(pg, m, r, g, b);
    unsigned char* o = out + i * 3;
    o[0] = (unsigned char)r;
    o[1] = (unsigned char)g;
    o[2] = (unsigned char)b;
  }
}

// The same program followed by the arithmetic and the store of image_crop_flip_normalize_kernel (input_pipeline.hip)
__global__ __launch_bounds__(256) void jitter_crop_flip_normalize_kernel(
    const unsigned char* __restrict__ img, int W, int x0, int y0, int cw, int ch, int flip, ssa_jitter_program pg,
    const unsigned long long* __restrict__ counter, Norm3 nm, bf16_t* __restrict__ out, int cpad) {
  const long n = (long)cw * ch;
  const int m = contrast_mean(pg, counter, n);
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int y = (int)(i / cw), x = (int)(i - (long)y * cw);
    const int sx = x0 + (flip ? cw - 1 - x : x), sy = y0 + y;
    const unsigned char* p = img + ((long)sy * W + sx) * 3;
    int c3[3] = {p[0], p[1], p[2]};
    jitter_pixel(pg, m, c3[0], c3[1], c3[2]);
    bf16_t* o = out + i * cpad;
    float f[8];
#pragma unroll
    for (int c = 0; c < 3; ++c) f[c] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)c3[c], 255.f), nm.mean[c]), nm.stdv[c]);
#pragma unroll
    for (int c = 3; c < 8; ++c) f[c] = 0.f;
    *reinterpret_cast<uint4*>(o) = pack8(f);
    for (int c0 = 8; c0 < cpad; c0 += 8) *reinterpret_cast<uint4*>(o + c0) = make_uint4(0, 0, 0, 0);
  }
}

bool window_ok(int H, int W, int x0, int y0, int cw, int ch) {
  return H > 0 && W > 0 && cw > 0 && ch > 0 && x0 >= 0 && y0 >= 0 && (long)x0 + cw <= W && (long)y0 + ch <= H;
}

// 0..4 distinct known op codes and finite factors (blend converts f * (x - d) + d to int: undefined for NaN and infinity);
// *has_contrast tells whether the program needs the luma sum
bool program_ok(const ssa_jitter_program* pg, bool* has_contrast) {
  if (!pg || pg->n_ops < 0 || pg->n_ops > 4 || pg->hue_byte < 0 || pg->hue_byte > 255) return false;
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(pg->factor[k])) return false;
  unsigned seen = 0;
  for (int k = 0; k < pg->n_ops; ++k) {
    const int op = pg->op[k];
    if (op < SSA_JITTER_BRIGHTNESS || op > SSA_JITTER_HUE || (seen >> op & 1u)) return false;
    seen |= 1u << op;
  }
  *has_contrast = seen >> SSA_JITTER_CONTRAST & 1u;
  return true;
}

int blocks_for(long n) { return (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096); }

}  // namespace

extern "C" {

int ssa_jitter_luma_sum(const unsigned char* img_hwc, int H, int W, int x0, int y0, int cw, int ch,
                        const ssa_jitter_program* program, unsigned long long* counter, void* stream) {
  bool contrast = false;
  if (!img_hwc || !program_ok(program, &contrast) || !window_ok(H, W, x0, y0, cw, ch)) return SSA_EINVAL;
  if (!contrast) return SSA_OK;                   // nothing reads the counter
  if (!counter || (reinterpret_cast<uintptr_t>(counter) & 7u)) return SSA_EINVAL;
  hipLaunchKernelGGL(jitter_clear_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, counter);
  SSA_LAUNCH_CHECK();
  hipLaunchKernelGGL(jitter_luma_sum_kernel, dim3(blocks_for((long)cw * ch)), dim3(256), 0, (hipStream_t)stream,
                     img_hwc, W, x0, y0, cw, ch, *program, counter);
  SSA_LAUNCH_CHECK();
  return SSA_OK;
}

int ssa_jitter_apply_u8(const unsigned char* img_hwc, int H, int W, int x0, int y0, int cw, int ch, int flip,
                        const ssa_jitter_program* program, const unsigned long long* counter,
                        unsigned char* out_hwc, void* stream) {
  bool contrast = false;
  if (!img_hwc || !out_hwc || !program_ok(program, &contrast) || !window_ok(H, W, x0, y0, cw, ch)) return SSA_EINVAL;
  if (contrast && (!counter || (reinterpret_cast<uintptr_t>(counter) & 7u))) return SSA_EINVAL;
  hipLaunchKernelGGL(jitter_apply_u8_kernel, dim3(blocks_for((long)cw * ch)), dim3(256), 0, (hipStream_t)stream,
                     img_hwc, W, x0, y0, cw, ch, flip ? 1 : 0, *program, counter, out_hwc);
  SSA_LAUNCH_CHECK();
  return SSA_OK;
}

int ssa_jitter_crop_flip_normalize(const unsigned char* img_hwc, int H, int W, int x0, int y0, int cw, int ch,
                                   int flip, const ssa_jitter_program* program, const unsigned long long* counter,
                                   const float* mean3, const float* std3, void* out_nhwc_bf16, int cpad,
                                   void* stream) {
  bool contrast = false;
  if (!img_hwc || !out_nhwc_bf16 || !mean3 || !std3 || !program_ok(program, &contrast) ||
      !window_ok(H, W, x0, y0, cw, ch))
    return SSA_EINVAL;
  if (contrast && (!counter || (reinterpret_cast<uintptr_t>(counter) & 7u))) return SSA_EINVAL;
  if (cpad < 8 || cpad % 8 || (reinterpret_cast<uintptr_t>(out_nhwc_bf16) & 15u)) return SSA_EINVAL;
  Norm3 nm;
  for (int c = 0; c < 3; ++c) {
    if (!(std3[c] > 0.f)) return SSA_EINVAL;
    nm.mean[c] = mean3[c];
    nm.stdv[c] = std3[c];
  }
  hipLaunchKernelGGL(jitter_crop_flip_normalize_kernel, dim3(blocks_for((long)cw * ch)), dim3(256), 0,
                     (hipStream_t)stream, img_hwc, W, x0, y0, cw, ch, flip ? 1 : 0, *program, counter, nm,
                     (bf16_t*)out_nhwc_bf16, cpad);
  SSA_LAUNCH_CHECK();
  return SSA_OK;
}

}  // extern "C"
