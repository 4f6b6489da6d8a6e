// Grouped 3x3 convolution with 1 < groups < C on NHWC 16-bit activations (gfx950): forward, data gradient and weight
// gradient of
//   nn.Conv2d(C, C, 3, stride, padding = dilation, dilation, groups = G, bias = False)    network/SEresnext.py:183-185
// conv2 of every SE-ResNeXt bottleneck (G = 32, Cg = C / G = 4, 8, 16, 32).  The real work is 9 Cg multiply-adds per output
// element: the kernels stay on the memory side of the roofline as long as the matrix pipe is not wasted by more than a
// few times, so the tile is v_mfma_f32_16x16x32 on a block-diagonal chunk of 16 channels -- no LDS, every operand
// fragment is loaded straight from global memory in the layout the instruction wants:
//
//   D[16 channels][16 pixels] += A[16 channels][32 k] B[32 k][16 pixels]
//   B  lane (pixel l & 15, k-group l >> 4) holds 8 consecutive k = 8 consecutive CHANNELS of one tap of its pixel: one
//      16-byte load from the NHWC tensor (zero for a tap out of bounds);
//   A  the filter of the wave's chunk, fp32 parameter -> 16-bit ONCE per wave, kept in registers for all its pixels;
//   D  lane holds 4 consecutive channels of its pixel: one 8-byte store.
//   Cg <= 16: a chunk's 16 output channels read the same 16 input channels (whole groups: 16 % Cg == 0); k = 2 taps x 16
//      channels, 5 MFMAs per 16 pixels (the 10th tap is zero), the filter block-diagonal inside the chunk -- the matrix
//      pipe does 16 / Cg x 10 / 9 of the real work (4.4x at Cg = 4, 1.1x at Cg = 16);
//   Cg == 32: k = the group's 32 channels of one tap, 9 MFMAs, no waste.
// forward    y = round16(sum w x); optionally sum y / sum y^2 of the values AS STORED into the [replica][2][C] fp64 table
//            (ssa_dwconv3x3's contract: the BatchNorm behind it needs no statistics pass).
// data grad  the same kernel with the filter transposed inside each group and the taps mirrored: dx[q] = sum over (tap,
//            oc) of w dy[(q + d - t d) / s]; stride 2 keeps only the taps of the right parity per pixel (a zero fragment
//            otherwise: the gather of the one stride-2 layer).
// weight grad  D[16 oc][16 ic] per tap, k = 32 output PIXELS: the fragments are gathered element by element (a lane's 8 k
//            are 8 pixels of one channel; a load instruction touches 4 pixels x 32 contiguous bytes).  Workgroups split
//            the pixel axis; their fp32 partial tiles go to `ws` and a second launch adds them in split order, picks
//            the groups' diagonal blocks and writes (or adds to) dw in the parameter's own [C][Cg][3][3] layout.
// The filter operand of the MFMA is 16-bit: rounding the fp32 parameter to the storage type is part of the contract.
#include "common.h"
#include "conv_epilogue.h"
#include "../../include/semseg_hip.h"

namespace {

constexpr int NT = 256, WAVES = NT / 64;
constexpr int kBlocks = 2048;        // workgroup cap of the forward / data-gradient grid (all channel tiles together)
constexpr int kWgBlocks = 1024;      // workgroup cap of the weight-gradient grid

struct GcArgs {
  const bf16_t* src; const float* w; bf16_t* out; double* stats;
  int B, Hs, Ws, lds, Hd, Wd, ldo, C, Cg, stride, dil;
};

// source coordinate of destination coordinate o for tap k (0..2) along one axis; false: no such source element
template <bool DGRAD>
__device__ __forceinline__ bool src_coord(int o, int k, int stride, int dil, int ns, int* s) {
  if (!DGRAD) {
    *s = o * stride - dil + k * dil;
    return (unsigned)*s < (unsigned)ns;
  }
  const int t = o + dil - k * dil;
  if (t < 0 || (stride == 2 && (t & 1))) return false;
  *s = stride == 2 ? t >> 1 : t;
  return *s < ns;
}

// fwd: src = x [B,Hs,Ws] -> out = y [B,Hd,Wd]; dgrad: src = dy [B,Hs,Ws] -> out = dx [B,Hd,Wd]
template <bool DGRAD, bool WIDE>
__global__ __launch_bounds__(NT) void gconv_kernel(const GcArgs a) {
  constexpr int NM = WIDE ? 9 : 5;
  const int lane = threadIdx.x & 63, col = lane & 15, kg = lane >> 4;
  const int chunk = blockIdx.y * WAVES + (threadIdx.x >> 6);
  const int C = a.C, Cg = a.Cg;
  if (chunk * 16 >= C) return;                                        // (wave-uniform: the ragged last tile)
  const int kbase = WIDE ? (chunk * 16) / 32 * 32 + kg * 8 : chunk * 16 + (kg & 1) * 8;
  // the filter fragments: row = channel chunk * 16 + col of the OUTPUT of this pass, k = the channel summed over
  bf16x8_t wf[NM];
  {
    const int rc = chunk * 16 + col;
#pragma unroll
    for (int m = 0; m < NM; ++m) {
      const int tap = WIDE ? m : 2 * m + (kg >> 1);
      float f[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int kc = kbase + j;
        const bool ok = tap < 9 && rc < C && kc < C && rc / Cg == kc / Cg;
        const int oc = DGRAD ? kc : rc, ic = DGRAD ? rc : kc;
        f[j] = ok ? a.w[((long)oc * Cg + ic % Cg) * 9 + tap] : 0.f;
      }
      wf[m] = __builtin_bit_cast(bf16x8_t, pack8(f));
    }
  }
  float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
  const long P = (long)a.B * a.Hd * a.Wd, units = (P + 15) / 16;
  const int rc0 = chunk * 16 + kg * 4;
  for (long u = blockIdx.x; u < units; u += gridDim.x) {
    const long p = u * 16 + col;
    const bool live = p < P;
    const long pc = live ? p : P - 1;
    const int ox = (int)(pc % a.Wd);
    const long t = pc / a.Wd;
    const int oy = (int)(t % a.Hd), b = (int)(t / a.Hd);
    const bf16_t* img = a.src + (long)b * a.Hs * a.Ws * a.lds + kbase;
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int m = 0; m < NM; ++m) {
      const int tap = WIDE ? m : 2 * m + (kg >> 1);
      const int kh = tap / 3, kw = tap - kh * 3;
      int sy, sx;
      uint4 raw = make_uint4(0, 0, 0, 0);
      if (live && tap < 9 && kbase < C && src_coord<DGRAD>(oy, kh, a.stride, a.dil, a.Hs, &sy) &&
          src_coord<DGRAD>(ox, kw, a.stride, a.dil, a.Ws, &sx))
        raw = *reinterpret_cast<const uint4*>(img + ((long)sy * a.Ws + sx) * a.lds);
      acc = ssa_mfma16(wf[m], __builtin_bit_cast(bf16x8_t, raw), acc);
    }
    if (live && rc0 < C) {
      uint2 q;
      q.x = f2bf_pair(acc[0], acc[1]);
      q.y = f2bf_pair(acc[2], acc[3]);
      *reinterpret_cast<uint2*>(a.out + p * a.ldo + rc0) = q;
      if (!DGRAD && a.stats) {
        float f[8];
        unpack8(make_uint4(q.x, q.y, 0, 0), f);
#pragma unroll
        for (int j = 0; j < 4; ++j) { s1[j] += f[j]; s2[j] += f[j] * f[j]; }
      }
    }
  }
  if (!DGRAD && a.stats) {
    double* st = a.stats + (long)(blockIdx.x % ssa::kStatReplicas) * 2 * C;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double d1 = (double)s1[j], d2 = (double)s2[j];
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) { d1 += __shfl_xor(d1, o, 64); d2 += __shfl_xor(d2, o, 64); }
      if (col == 0 && rc0 + j < C) { atomicAdd(&st[rc0 + j], d1); atomicAdd(&st[C + rc0 + j], d2); }
    }
  }
}

// Weight gradient.  A wave owns one 16 x 16 tile (oc chunk, ic block) and all nine taps: D_t[oc][ic] += sum over 32
// output pixels of dy[o][oc] x[src(o, t)][ic].  tile -> (chunk, icb): Cg == 32 has two ic blocks per chunk (the group's
// two halves), else the ic block is the chunk's own 16 channels.
struct GwArgs {
  const bf16_t* x; const bf16_t* dy; float* ws;
  int B, H, W, ldx, Ho, Wo, ldg, C, Cg, stride, dil, ntile;
};

__global__ __launch_bounds__(NT) void gconv_wgrad_kernel(const GwArgs a) {
  const int lane = threadIdx.x & 63, col = lane & 15, kg = lane >> 4;
  const int tile = blockIdx.y * WAVES + (threadIdx.x >> 6);
  if (tile >= a.ntile) return;                                        // (wave-uniform)
  const bool wide = a.Cg == 32;
  const int chunk = wide ? tile >> 1 : tile;
  const int oc = chunk * 16 + col;                                    // A: row = oc
  const int ic = (wide ? chunk * 16 / 32 * 32 + (tile & 1) * 16 : chunk * 16) + col;   // B: column = ic
  const bool oc_ok = oc < a.C, ic_ok = ic < a.C;
  f32x4_t acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const long P = (long)a.B * a.Ho * a.Wo, steps = (P + 31) / 32;
  for (long ks = blockIdx.x; ks < steps; ks += gridDim.x) {
    const long q0 = ks * 32 + kg * 8;
    // (b, oy, ox) of the lane's first pixel; the other seven follow by increments
    long r = q0 < P ? q0 : 0;
    int ox = (int)(r % a.Wo);
    r /= a.Wo;
    int oy = (int)(r % a.Ho), b = (int)(r / a.Ho);
    bf16_t av[8], bv[9][8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bool live = q0 + j < P;
      av[j] = live && oc_ok ? a.dy[(q0 + j) * a.ldg + oc] : (bf16_t)0;
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int kh = t / 3, kw = t - kh * 3;
        int sy, sx;
        bf16_t v = 0;
        if (live && ic_ok && src_coord<false>(oy, kh, a.stride, a.dil, a.H, &sy) &&
            src_coord<false>(ox, kw, a.stride, a.dil, a.W, &sx))
          v = a.x[(((long)b * a.H + sy) * a.W + sx) * a.ldx + ic];
        bv[t][j] = v;
      }
      if (++ox == a.Wo) { ox = 0; if (++oy == a.Ho) { oy = 0; ++b; } }
    }
    uint4 qa;
    qa.x = av[0] | ((uint32_t)av[1] << 16); qa.y = av[2] | ((uint32_t)av[3] << 16);
    qa.z = av[4] | ((uint32_t)av[5] << 16); qa.w = av[6] | ((uint32_t)av[7] << 16);
    const bf16x8_t af = __builtin_bit_cast(bf16x8_t, qa);
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      uint4 qb;
      qb.x = bv[t][0] | ((uint32_t)bv[t][1] << 16); qb.y = bv[t][2] | ((uint32_t)bv[t][3] << 16);
      qb.z = bv[t][4] | ((uint32_t)bv[t][5] << 16); qb.w = bv[t][6] | ((uint32_t)bv[t][7] << 16);
      acc[t] = ssa_mfma16(af, __builtin_bit_cast(bf16x8_t, qb), acc[t]);
    }
  }
  // D: column (ic) = lane & 15, rows (oc) 4 (lane >> 4) + j
  float* dst = a.ws + ((long)blockIdx.x * a.ntile + tile) * 9 * 256;
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j) dst[t * 256 + (kg * 4 + j) * 16 + col] = acc[t][j];
}

// dw[oc][icl][t] (+)= sum over the splits' partial tiles, in split order
__global__ __launch_bounds__(NT) void gconv_wsum_kernel(const float* __restrict__ ws, int nsplit, int ntile, int C, int Cg,
                                                        float* __restrict__ dw, int accumulate) {
  const long e = blockIdx.x * (long)NT + threadIdx.x;
  if (e >= (long)C * Cg * 9) return;
  const int t = (int)(e % 9);
  const long r = e / 9;
  const int icl = (int)(r % Cg), oc = (int)(r / Cg);
  const int chunk = oc >> 4, row = oc & 15;
  const int tile = Cg == 32 ? chunk * 2 + (icl >> 4) : chunk;
  const int colc = Cg == 32 ? icl & 15 : (oc / Cg * Cg + icl) & 15;
  const float* src = ws + ((long)tile * 9 + t) * 256 + row * 16 + colc;
  float s = 0.f;
  for (int k = 0; k < nsplit; ++k) s += src[(long)k * ntile * 9 * 256];
  dw[e] = accumulate ? dw[e] + s : s;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// -1: a bad descriptor; -2: a form the kernels are not built for; 0: fine
int check_desc(const ssa_gconv_desc* d) {
  if (!d || d->B < 1 || d->H < 1 || d->W < 1 || d->C < 8 || d->C % 8 || d->G < 1 || d->C % d->G) return SSA_EINVAL;
  if (d->ldx < d->C || d->ldy < d->C || d->ldx % 8 || d->ldy % 8) return SSA_EINVAL;
  if (!((d->stride == 1 && d->dil >= 1) || (d->stride == 2 && d->dil == 1))) return SSA_EINVAL;
  if (d->Ho != (d->H - 1) / d->stride + 1 || d->Wo != (d->W - 1) / d->stride + 1) return SSA_EINVAL;
  if ((double)d->B * d->H * d->W >= 2147483648.0) return SSA_EINVAL;
  const int Cg = d->C / d->G;
  if (Cg != 4 && Cg != 8 && Cg != 16 && Cg != 32) return SSA_EUNSUPPORTED;
  return SSA_OK;
}

dim3 plan_grid(int C, long pixels) {
  const int ny = ((C + 15) / 16 + WAVES - 1) / WAVES;
  const long units = (pixels + 15) / 16, most = kBlocks / ny > 1 ? kBlocks / ny : 1;
  return dim3((unsigned)(units < most ? units : most), (unsigned)ny);
}

struct WgPlan { int ntile, ny, nsplit; };
WgPlan plan_wgrad(const ssa_gconv_desc& d) {
  WgPlan p;
  p.ntile = (d.C + 15) / 16 * (d.C / d.G == 32 ? 2 : 1);
  p.ny = (p.ntile + WAVES - 1) / WAVES;
  const long steps = ((long)d.B * d.Ho * d.Wo + 31) / 32, most = kWgBlocks / p.ny > 1 ? kWgBlocks / p.ny : 1;
  p.nsplit = (int)(steps < most ? steps : most);
  return p;
}

template <bool DGRAD>
void launch(const GcArgs& a, dim3 grid, hipStream_t s) {
  if (a.Cg == 32) hipLaunchKernelGGL((gconv_kernel<DGRAD, true>), grid, dim3(NT), 0, s, a);
  else hipLaunchKernelGGL((gconv_kernel<DGRAD, false>), grid, dim3(NT), 0, s, a);
}

}  // namespace

extern "C" {

int ssa_gconv3x3(const ssa_gconv_desc* d, const void* x, const float* w, void* y, double* stats, void* stream) {
  if (const int rc = check_desc(d)) return rc;
  if (!x || !w || !y || !aligned16(x) || !aligned16(y)) return SSA_EINVAL;
  const GcArgs a = {(const bf16_t*)x, w, (bf16_t*)y, stats, d->B, d->H, d->W, d->ldx, d->Ho, d->Wo, d->ldy,
                    d->C, d->C / d->G, d->stride, d->dil};
  launch<false>(a, plan_grid(d->C, (long)d->B * d->Ho * d->Wo), (hipStream_t)stream);
  SSA_LAUNCH_CHECK();
  return SSA_OK;
}

int ssa_gconv3x3_bwd_plan(const ssa_gconv_desc* d, size_t* ws_bytes) {
  if (const int rc = check_desc(d)) return rc;
  if (!ws_bytes) return SSA_EINVAL;
  const WgPlan p = plan_wgrad(*d);
  *ws_bytes = (size_t)p.nsplit * p.ntile * 9 * 256 * sizeof(float);
  return SSA_OK;
}

int ssa_gconv3x3_bwd(const ssa_gconv_desc* d, const void* x, const void* dy, int lddy, const float* w, void* dx, int lddx,
                     float* dw, int accumulate, void* ws, void* stream) {
  if (const int rc = check_desc(d)) return rc;
  if (!dy || (!dx && !dw) || lddy < d->C || lddy % 8 || !aligned16(dy)) return SSA_EINVAL;
  if (dx && (!w || lddx < d->C || lddx % 8 || !aligned16(dx))) return SSA_EINVAL;
  if (dw && (!x || !ws || !aligned16(x))) return SSA_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (dx) {
    const GcArgs a = {(const bf16_t*)dy, w, (bf16_t*)dx, nullptr, d->B, d->Ho, d->Wo, lddy, d->H, d->W, lddx,
                      d->C, d->C / d->G, d->stride, d->dil};
    launch<true>(a, plan_grid(d->C, (long)d->B * d->H * d->W), s);
    SSA_LAUNCH_CHECK();
  }
  if (dw) {
    const WgPlan p = plan_wgrad(*d);
    const GwArgs g = {(const bf16_t*)x, (const bf16_t*)dy, (float*)ws, d->B, d->H, d->W, d->ldx, d->Ho, d->Wo, lddy,
                      d->C, d->C / d->G, d->stride, d->dil, p.ntile};
    hipLaunchKernelGGL(gconv_wgrad_kernel, dim3(p.nsplit, p.ny), dim3(NT), 0, s, g);
    SSA_LAUNCH_CHECK();
    const long n = (long)d->C * (d->C / d->G) * 9;
    hipLaunchKernelGGL(gconv_wsum_kernel, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, s, (const float*)ws, p.nsplit,
                       p.ntile, d->C, d->C / d->G, dw, accumulate ? 1 : 0);
    SSA_LAUNCH_CHECK();
  }
  return SSA_OK;
}

}  // extern "C"
