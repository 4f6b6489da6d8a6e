// What the entry points of the image half of the input tail share (input_pipeline.hip, color_jitter.hip, gblur.hip),
// stated once: the normalise arithmetic and its 16-byte stores, the streaming kernel over a crop window with or
// without a ColorJitter program (jitter_device.h keeps the per-pixel arithmetic of the program) and with a byte or a
// normalised store, and the host-side checks and grid rule of its launches.
#pragma once
#include "jitter_device.h"

namespace {

struct Norm3 { float mean[3], stdv[3]; };

// bf16(((float)u8 / 255 - mean[c]) / std[c]) of the three channels, zeros up to cpad (a multiple of 8), as 16-byte
// pieces at o.  Divisions and a subtraction rounded on their own and no multiply next to an add: it means the same in a
// file compiled under fp contract(off) and in one compiled under the default.
__device__ __forceinline__ void store_normalized(int r, int g, int b, const Norm3& nm, bf16_t* o, int cpad) {
  const int c3[3] = {r, g, b};
  float f[8];
#pragma unroll
  for (int c = 0; c < 3; ++c) f[c] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)c3[c], 255.f), nm.mean[c]), nm.stdv[c]);
#pragma unroll
  for (int c = 3; c < 8; ++c) f[c] = 0.f;
  *reinterpret_cast<uint4*>(o) = pack8(f);
  for (int c0 = 8; c0 < cpad; c0 += 8) *reinterpret_cast<uint4*>(o + c0) = make_uint4(0, 0, 0, 0);
}

// One pixel of the window per thread and step: the mirrored source pixel, through the program (JITTER; the contrast
// mean read from the counter ssa_jitter_luma_sum left) or as it is (pg and counter are not read), stored as three bytes
// or normalised (NORM).  The program and the counter come last: what the other arguments and the grid size occupy then
// ends within 128 bytes, as the argument block of a kernel without them would.
template <bool JITTER, bool NORM>
__global__ __launch_bounds__(256) void tail_stream_kernel(const unsigned char* __restrict__ img, int W, int x0, int y0,
                                                          int cw, int ch, int flip, Norm3 nm, void* __restrict__ out,
                                                          int cpad, ssa_jitter_program pg,
                                                          const unsigned long long* __restrict__ counter) {
  const long n = (long)cw * ch;
  int m = 0;
  if (JITTER) m = contrast_mean(pg, counter, n);
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int y = (int)(i / cw), x = (int)(i - (long)y * cw);
    const int sx = x0 + (flip ? cw - 1 - x : x), sy = y0 + y;
    const unsigned char* p = img + ((long)sy * W + sx) * 3;
    int r = p[0], g = p[1], b = p[2];
    if (JITTER) jitter_pixel(pg, m, r, g, b);
    if (NORM) {
      store_normalized(r, g, b, nm, (bf16_t*)out + i * cpad, cpad);
    } else {
      unsigned char* o = (unsigned char*)out + i * 3;
      o[0] = (unsigned char)r;
      o[1] = (unsigned char)g;
      o[2] = (unsigned char)b;
    }
  }
}

bool window_ok(int H, int W, int x0, int y0, int cw, int ch) {
  return H > 0 && W > 0 && cw > 0 && ch > 0 && x0 >= 0 && y0 >= 0 && (long)x0 + cw <= W && (long)y0 + ch <= H;
}

// Workgroups of 256 for n pixels under a grid-stride loop
int stream_blocks(long n) { return (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096); }

// mean, positive std, a padded channel count that is a multiple of 8 and a 16-byte aligned output -> *nm
bool norm3_ok(const float* mean3, const float* std3, const void* out, int cpad, Norm3* nm) {
  if (!mean3 || !std3 || cpad < 8 || cpad % 8 || (reinterpret_cast<uintptr_t>(out) & 15u)) return false;
  for (int c = 0; c < 3; ++c) {
    if (!(std3[c] > 0.f)) return false;
    nm->mean[c] = mean3[c];
    nm->stdv[c] = std3[c];
  }
  return true;
}

template <bool JITTER, bool NORM>
int tail_stream_launch(const unsigned char* img, int W, int x0, int y0, int cw, int ch, int flip, const Norm3& nm,
                       void* out, int cpad, const ssa_jitter_program& pg, const unsigned long long* counter,
                       void* stream) {
  hipLaunchKernelGGL((tail_stream_kernel<JITTER, NORM>), dim3(stream_blocks((long)cw * ch)), dim3(256), 0,
                     (hipStream_t)stream, img, W, x0, y0, cw, ch, flip ? 1 : 0, nm, out, cpad, pg, counter);
  SSA_LAUNCH_CHECK();
  return SSA_OK;
}

}  // namespace
