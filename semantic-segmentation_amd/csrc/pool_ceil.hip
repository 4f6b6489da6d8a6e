// nn.MaxPool2d(3, stride=2, ceil_mode=True), no padding, on NHWC 16-bit activations (gfx950): the stem pool of the
// SE-ResNeXt trunks (network/SEresnext.py:271-272).  Window of output (oy, ox): rows 2 oy .. 2 oy + 2, columns
// 2 ox .. 2 ox + 2, clipped to the image (a tap past the edge never wins); Ho = H / 2, Wo = W / 2 for H, W >= 2.  The
// first-maximum / NaN rule and the byte index map (tap = kh * 3 + kw per channel) are those of pool.hip's padding-1
// kernels, whose entry points stay as they are.  HBM-bound streaming kernels: one thread owns one 16-byte channel group.
#include "common.h"
#include "../../include/semseg_hip.h"

namespace {

__global__ __launch_bounds__(256) void maxpoolc_fwd_kernel(const bf16_t* __restrict__ x, int ldx, int B, int H, int W,
                                                           int C, bf16_t* __restrict__ y, unsigned char* __restrict__ idx,
                                                           int Ho, int Wo) {
  const int VC = C >> 3;
  const long n = (long)B * Ho * Wo * VC;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int cg = (int)(i % VC);
    long p = i / VC;
    const int ox = (int)(p % Wo); p /= Wo;
    const int oy = (int)(p % Ho);
    const int b = (int)(p / Ho);
    float best[8];
    int arg[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { best[j] = -INFINITY; arg[j] = -1; }
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int iy = oy * 2 + kh, ix = ox * 2 + kw;
        if (iy >= H || ix >= W) continue;
        float f[8];
        unpack8(*reinterpret_cast<const uint4*>(x + ((long)(b * H + iy) * W + ix) * ldx + cg * 8), f);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if (arg[j] < 0) arg[j] = kh * 3 + kw;                 // first in-bounds tap (always tap 0 here)
          if (f[j] > best[j] || f[j] != f[j]) { best[j] = f[j]; arg[j] = kh * 3 + kw; }
        }
      }
    const long o = ((long)(b * Ho + oy) * Wo + ox) * C + cg * 8;
    *reinterpret_cast<uint4*>(y + o) = pack8(best);
    uint2 a;
    a.x = (unsigned)arg[0] | ((unsigned)arg[1] << 8) | ((unsigned)arg[2] << 16) | ((unsigned)arg[3] << 24);
    a.y = (unsigned)arg[4] | ((unsigned)arg[5] << 8) | ((unsigned)arg[6] << 16) | ((unsigned)arg[7] << 24);
    *reinterpret_cast<uint2*>(idx + o) = a;
  }
}

// backward as a gather (deterministic, no atomics): an input pixel collects dy from the (at most four) windows that
// cover it and whose stored argmax is this pixel; a pixel no window covers (the last row / column of an odd size is
// always covered: 2 (Ho - 1) + 2 >= H - 1) gets zero
__global__ __launch_bounds__(256) void maxpoolc_bwd_kernel(const bf16_t* __restrict__ dy,
                                                           const unsigned char* __restrict__ idx, int B, int Ho, int Wo,
                                                           int C, bf16_t* __restrict__ dx, int H, int W) {
  const int VC = C >> 3;
  const long n = (long)B * H * W * VC;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int cg = (int)(i % VC);
    long p = i / VC;
    const int ix = (int)(p % W); p /= W;
    const int iy = (int)(p % H);
    const int b = (int)(p / H);
    float g[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) g[j] = 0.f;
    // windows oy with 2 oy <= iy <= 2 oy + 2
    const int oy0 = iy >= 2 ? (iy - 1) >> 1 : 0, ox0 = ix >= 2 ? (ix - 1) >> 1 : 0;
    for (int oy = oy0; oy <= iy >> 1; ++oy)
      for (int ox = ox0; ox <= ix >> 1; ++ox) {
        if (oy >= Ho || ox >= Wo) continue;
        const int tap = (iy - oy * 2) * 3 + (ix - ox * 2);
        const long o = ((long)(b * Ho + oy) * Wo + ox) * C + cg * 8;
        const uint2 a = *reinterpret_cast<const uint2*>(idx + o);
        float d[8];
        unpack8(*reinterpret_cast<const uint4*>(dy + o), d);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const unsigned t = ((j < 4 ? a.x : a.y) >> (8 * (j & 3))) & 0xffu;
          if ((int)t == tap) g[j] += d[j];
        }
      }
    *reinterpret_cast<uint4*>(dx + ((long)(b * H + iy) * W + ix) * C + cg * 8) = pack8(g);
  }
}

int grid_for(long n) { return (int)((n + 255) / 256 > 16384 ? 16384 : (n + 255) / 256); }
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int ssa_maxpool3x3s2c_fwd(const void* x, int ldx, int B, int H, int W, int C, void* y, unsigned char* idx, int Ho,
                          int Wo, void* stream) {
  if (!x || !y || !idx || C < 8 || C % 8 || ldx % 8 || ldx < C || B < 1 || H < 2 || W < 2 || Ho != H / 2 || Wo != W / 2)
    return SSA_EINVAL;
  if (!aligned16(x) || !aligned16(y) || ((uintptr_t)idx & 7)) return SSA_EINVAL;
  const long n = (long)B * Ho * Wo * (C >> 3);
  hipLaunchKernelGGL(maxpoolc_fwd_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, ldx, B,
                     H, W, C, (bf16_t*)y, idx, Ho, Wo);
  SSA_LAUNCH_CHECK();
  return SSA_OK;
}

int ssa_maxpool3x3s2c_bwd(const void* dy, const unsigned char* idx, int B, int Ho, int Wo, int C, void* dx, int H, int W,
                          void* stream) {
  if (!dy || !idx || !dx || C < 8 || C % 8 || B < 1 || H < 2 || W < 2 || Ho != H / 2 || Wo != W / 2) return SSA_EINVAL;
  if (!aligned16(dy) || !aligned16(dx) || ((uintptr_t)idx & 7)) return SSA_EINVAL;
  const long n = (long)B * H * W * (C >> 3);
  hipLaunchKernelGGL(maxpoolc_bwd_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)dy, idx, B,
                     Ho, Wo, C, (bf16_t*)dx, H, W);
  SSA_LAUNCH_CHECK();
  return SSA_OK;
}

}  // extern "C"
