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
#include "jitter_device.h"

// Every product and sum in this file is rounded on its own, as the C code Pillow was compiled from rounds them: no
// contraction to FMA.  hipcc contracts by default, across statements and through inlined functions, and the
// __fmul_rn / __fadd_rn of the HIP headers do not stop it: they are inline functions over the plain operators, compiled
// under the default, so d + f * (x - d) written with them still came out as one v_fma_f32 (0.8 * -145 + 147 = 30.999998
// instead of 31).  Hence plain operators under this pragma for every multiply, add and subtract below.
#pragma clang fp contract(off)

namespace {

struct Norm3 { float mean[3], stdv[3]; };

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
