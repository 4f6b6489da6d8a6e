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
#include "input_tail.h"

// Every product and sum in this file is rounded on its own, as the C code Pillow was compiled from rounds them: no
// contraction to FMA.  hipcc contracts by default, across statements and through inlined functions, and the
// __fmul_rn / __fadd_rn of the HIP headers do not stop it: they are inline functions over the plain operators, compiled
// under the default, so d + f * (x - d) written with them still came out as one v_fma_f32 (0.8 * -145 + 147 = 30.999998
// instead of 31).  Hence plain operators under this pragma for every multiply, add and subtract below.
#pragma clang fp contract(off)

namespace {

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
  hipLaunchKernelGGL(jitter_luma_sum_kernel, dim3(stream_blocks((long)cw * ch)), dim3(256), 0, (hipStream_t)stream,
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
  return tail_stream_launch<true, false>(img_hwc, W, x0, y0, cw, ch, flip, Norm3{}, out_hwc, 0, *program, counter,
                                         stream);
}

int ssa_jitter_crop_flip_normalize(const unsigned char* img_hwc, int H, int W, int x0, int y0, int cw, int ch,
                                   int flip, const ssa_jitter_program* program, const unsigned long long* counter,
                                   const float* mean3, const float* std3, void* out_nhwc_bf16, int cpad,
                                   void* stream) {
  bool contrast = false;
  Norm3 nm;
  if (!img_hwc || !out_nhwc_bf16 || !program_ok(program, &contrast) || !window_ok(H, W, x0, y0, cw, ch) ||
      !norm3_ok(mean3, std3, out_nhwc_bf16, cpad, &nm))
    return SSA_EINVAL;
  if (contrast && (!counter || (reinterpret_cast<uintptr_t>(counter) & 7u))) return SSA_EINVAL;
  return tail_stream_launch<true, true>(img_hwc, W, x0, y0, cw, ch, flip, nm, out_nhwc_bf16, cpad, *program, counter,
                                        stream);
}

}  // extern "C"
