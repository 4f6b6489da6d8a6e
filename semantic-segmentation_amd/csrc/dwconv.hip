// Depthwise 3x3 convolution on NHWC 16-bit activations (gfx950): forward, data gradient and weight gradient of
//   nn.Conv2d(C, C, 3, stride, padding = dilation, dilation, groups = C, bias = False)    network/xception.py:30-32
// the first half of every SeparableConv2d of the Xception-71 trunk.  No MFMA work: a stencil of 9 FMAs per element that
// streams from HBM.  One lane owns one 16-byte channel group (pool.hip / bn.hip) and a short RUN of pixels along x: its
// 72 weights ([C][9] fp32, the parameter's own storage) are loaded once per kernel, and the source columns a run needs
// are loaded once per row and shared by the taps that fall on them (6 columns for 4 outputs x 3 taps at dilation 1).
//
// forward   y = round16(sum_t w[t] x[o * s - d + t * d]); optionally sum y / sum y^2 of the values AS STORED into a
//           [replica][2][C] fp64 table (the ssa_bn_stats pass of the BatchNorm behind it), or, inference, that BatchNorm
//           itself: z = round16(scale * round16(y) + shift), ReLU.
// backward  a gather over the INPUT pixels q: every (output o, tap t) pair belongs to exactly one q = o * s - d + t * d, so
//           one pass gives dx[q] = sum_t w[t] dy[o(q, t)] and dW[t] += x[q] dy[o(q, t)] from one read of dy and of x.  No
//           atomics: dW is summed per thread, per workgroup (LDS), and across workgroups as fp32 partials in `ws` that a
//           second small launch adds up in a fixed order.  Stride 2: only the taps of the right parity exist for a pixel
//           (maxpool_bwd_kernel's rule).
#include "common.h"
#include "conv_epilogue.h"
#include "../../include/semseg_hip.h"

namespace {

constexpr int NT = 256;
constexpr int kRunFwd = 4;       // output pixels per thread and unit, forward
constexpr int kRunBwd = 2;       // input pixels per thread and unit, backward (72 more accumulators live: dW)
constexpr int kTile = 16;        // channel groups (256 bytes of a pixel) per workgroup: 16 x 16 lanes = 16 runs at a time
// Workgroup caps (all channel tiles together): past them a workgroup walks several units.  The kernels hold 200-250
// registers, two workgroups per CU: 512 are resident at once, and a thread that lives long pays its 72 weights, and in
// backward the nine block reductions and 36 C bytes of partial sums, once for many pixels.
constexpr int kFwdBlocks = 1024, kBwdBlocks = 512;

// lane -> (channel group, pixel row) of a workgroup: blockIdx.y picks a tile of TW = min(C / 8, kTile) channel groups,
// the NT / TW rows of threads each own a run
struct Lane {
  int TW, RP, cg, pr;
  bool active;
  __device__ __forceinline__ Lane(int C) {
    const int VC = C >> 3, t = threadIdx.x;
    TW = VC < kTile ? VC : kTile;
    RP = NT / TW;
    pr = t / TW;
    const int g = blockIdx.y * TW + t % TW;
    active = pr < RP && g < VC;
    cg = g < VC ? g : VC - 1;          // (an idle lane of the ragged last tile loads the last group's weights)
  }
};

// Which source column j of a run's window serves (pixel r of the run, tap kw).  DIL = 0: dilation known at run time
// only, no sharing (column j = 3 r + kw).
template <int S, int DIL, int R> struct FwdMap {        // source x of output x0 + r, tap kw: (x0 + r) S + (kw - 1) d
  static constexpr int NCOL = DIL ? (R - 1) * S + 2 * DIL + 1 : 3 * R;
  static __device__ __forceinline__ int col(int x0, int j, int dil) {
    return DIL ? x0 * S - DIL + j : (x0 + j / 3) * S + (j % 3 - 1) * dil;
  }
  static constexpr bool hit(int j, int r, int kw) { return DIL ? r * S + kw * DIL == j : j == r * 3 + kw; }
  static __device__ __forceinline__ bool row(int y, int kh, int dil, int* sy) { *sy = y * S + (kh - 1) * dil; return true; }
};
template <int S, int DIL, int R> struct BwdMap {        // output x of input x0 + r, tap kw: (x0 + r + d - kw d) / S
  static_assert(S == 1 || (DIL == 1 && R % 2 == 0), "stride 2: dilation 1, runs start at an even x");
  static constexpr int NCOL = S == 2 ? R / 2 + 1 : (DIL ? R - 1 + 2 * DIL + 1 : 3 * R);
  static __device__ __forceinline__ int col(int x0, int j, int dil) {
    return S == 2 ? (x0 >> 1) + j : (DIL ? x0 - DIL + j : x0 + j / 3 - (j % 3 - 1) * dil);
  }
  static constexpr bool hit(int j, int r, int kw) {
    return S == 2 ? r + 1 - kw == 2 * j : (DIL ? r + (2 - kw) * DIL == j : j == r * 3 + kw);
  }
  static __device__ __forceinline__ bool row(int y, int kh, int dil, int* sy) {
    if (S == 2) { const int d = y + 1 - kh; *sy = d >> 1; return d >= 0 && !(d & 1); }
    *sy = y - (kh - 1) * dil;
    return true;
  }
};

struct DwArgs {
  const bf16_t* x; const bf16_t* g; const float* w; bf16_t* out; double* stats; const float* coef; float* ws;
  int B, H, W, C, ldx, Ho, Wo, ldg, ldo, dil, relu;
};

// acc[r] += w[t] src[..], and with DW dw[t] += xq[r] src[..], over the 3 x NCOL window of the run (x0 .. x0 + R - 1) of
// row y; src: the image's first pixel + this lane's channel group, Hs x Ws pixels of stride ld
template <class M, int R, bool ACC, bool DW>
__device__ __forceinline__ void gather_run(const bf16_t* __restrict__ src, int ld, int Hs, int Ws, int y, int x0, int dil,
                                           const float (&w)[9][8], float (&acc)[R][8], const float (&xq)[R][8],
                                           float (&dw)[9][8]) {
#pragma unroll
  for (int kh = 0; kh < 3; ++kh) {
    int sy;
    if (!M::row(y, kh, dil, &sy) || (unsigned)sy >= (unsigned)Hs) continue;
    const bf16_t* rowp = src + (long)sy * Ws * ld;
    uint4 raw[M::NCOL];
#pragma unroll
    for (int j = 0; j < M::NCOL; ++j) {
      const int sx = M::col(x0, j, dil);
      raw[j] = (unsigned)sx < (unsigned)Ws ? *reinterpret_cast<const uint4*>(rowp + (long)sx * ld) : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < M::NCOL; ++j) {
      float f[8];
      unpack8(raw[j], f);
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw)
          if (M::hit(j, r, kw)) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
              if (ACC) acc[r][i] += w[kh * 3 + kw][i] * f[i];
              if (DW) dw[kh * 3 + kw][i] += xq[r][i] * f[i];
            }
          }
    }
  }
}

// The forward's form: no dW operands (the two stand-ins are never touched with DW = false and cost no register)
template <class M, int R>
__device__ __forceinline__ void gather_fwd(const bf16_t* __restrict__ src, int ld, int Hs, int Ws, int y, int x0, int dil,
                                           const float (&w)[9][8], float (&acc)[R][8]) {
  const float no_xq[R][8] = {};
  float no_dw[9][8];
  gather_run<M, R, true, false>(src, ld, Hs, Ws, y, x0, dil, w, acc, no_xq, no_dw);
}

// Sum over the pixel rows of a workgroup: v of thread (pr, cg) -> f(channel, sum) on one thread per channel.  Every thread
// of the workgroup calls it (idle ones with zeros).
template <class F>
__device__ __forceinline__ void reduce_rows(const float (&v)[8], float* red, const Lane& ln, int C, F f) {
  const int t = threadIdx.x;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 8; ++i) red[t * 9 + i] = v[i];
  __syncthreads();
  if (t < ln.TW * 8) {
    const int g = t >> 3, i = t & 7;
    const int c = (blockIdx.y * ln.TW + g) * 8 + i;
    if (c < C) {
      double s = 0.0;
      for (int p = 0; p < ln.RP; ++p) s += (double)red[(p * ln.TW + g) * 9 + i];
      f(c, s);
    }
  }
}

__device__ __forceinline__ void load_weights(const float* __restrict__ w, int cg, float (&wr)[9][8]) {
  // 8 channels x 9 taps are 72 consecutive floats, 288 bytes: 18 16-byte loads
  float4 v[18];
#pragma unroll
  for (int k = 0; k < 18; ++k) v[k] = reinterpret_cast<const float4*>(w + cg * 72)[k];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int e = i * 9 + t;
      const float4& q = v[e >> 2];
      wr[t][i] = (e & 3) == 0 ? q.x : ((e & 3) == 1 ? q.y : ((e & 3) == 2 ? q.z : q.w));
    }
}

template <int S, int DIL>
__global__ __launch_bounds__(NT) void dwconv_fwd_kernel(const DwArgs a) {
  constexpr int R = kRunFwd;
  typedef FwdMap<S, DIL, R> M;
  __shared__ float red[NT * 9];
  const Lane ln(a.C);
  const int cg = ln.cg, pr = ln.pr, RP = ln.RP;
  const bool active = ln.active;
  float w[9][8], s1[8], s2[8], sc[8], sh[8];
  load_weights(a.w, cg, w);
#pragma unroll
  for (int i = 0; i < 8; ++i) { s1[i] = 0.f; s2[i] = 0.f; sc[i] = 1.f; sh[i] = 0.f; }
  if (a.coef) {
#pragma unroll
    for (int i = 0; i < 8; ++i) { sc[i] = a.coef[cg * 8 + i]; sh[i] = a.coef[a.C + cg * 8 + i]; }
  }
  const int runs_x = (a.Wo + R - 1) / R;
  const long nrun = (long)a.B * a.Ho * runs_x;
  if (active)
    for (long u = (long)blockIdx.x * RP + pr; u < nrun; u += (long)gridDim.x * RP) {
      const int x0 = (int)(u % runs_x) * R;
      const long p = u / runs_x;
      const int oy = (int)(p % a.Ho), b = (int)(p / a.Ho);
      float acc[R][8];
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[r][i] = 0.f;
      gather_fwd<M, R>(a.x + (long)b * a.H * a.W * a.ldx + cg * 8, a.ldx, a.H, a.W, oy, x0, a.dil, w, acc);
      bf16_t* yo = a.out + ((long)(b * a.Ho + oy) * a.Wo + x0) * a.ldo + cg * 8;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (x0 + r >= a.Wo) break;
        uint4 q = pack8(acc[r]);
        if (a.stats || a.coef) {
          float f[8];
          unpack8(q, f);
          if (a.stats) {
#pragma unroll
            for (int i = 0; i < 8; ++i) { s1[i] += f[i]; s2[i] += f[i] * f[i]; }
          } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) f[i] = f[i] * sc[i] + sh[i];
            if (a.relu) {
#pragma unroll
              for (int i = 0; i < 8; ++i) f[i] = fmaxf(f[i], 0.f);
            }
            q = pack8(f);
          }
        }
        *reinterpret_cast<uint4*>(yo + (long)r * a.ldo) = q;
      }
    }
  if (a.stats) {
    double* st = a.stats + (long)(blockIdx.x % ssa::kStatReplicas) * 2 * a.C;
    const int C = a.C;
    reduce_rows(s1, red, ln, C, [=](int c, double s) { atomicAdd(&st[c], s); });
    reduce_rows(s2, red, ln, C, [=](int c, double s) { atomicAdd(&st[C + c], s); });
  }
}

// x: the forward's input, g: dy ([B,Ho,Wo,C], stride ldg), out: dx ([B,H,W,C], stride ldo), ws: [gridDim.x][9][C] fp32
template <int S, int DIL, bool DX, bool DW>
__global__ __launch_bounds__(NT) void dwconv_bwd_kernel(const DwArgs a) {
  constexpr int R = kRunBwd;
  typedef BwdMap<S, DIL, R> M;
  __shared__ float red[NT * 9];
  const Lane ln(a.C);
  const int cg = ln.cg, pr = ln.pr, RP = ln.RP;
  const bool active = ln.active;
  float w[9][8], dw[9][8];
  load_weights(a.w, cg, w);
#pragma unroll
  for (int k = 0; k < 9; ++k)
#pragma unroll
    for (int i = 0; i < 8; ++i) dw[k][i] = 0.f;
  const int runs_x = (a.W + R - 1) / R;
  const long nrun = (long)a.B * a.H * runs_x;
  if (active)
    for (long u = (long)blockIdx.x * RP + pr; u < nrun; u += (long)gridDim.x * RP) {
      const int x0 = (int)(u % runs_x) * R;
      const long p = u / runs_x;
      const int iy = (int)(p % a.H), b = (int)(p / a.H);
      float acc[R][8], xq[R][8];
#pragma unroll
      for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int i = 0; i < 8; ++i) { acc[r][i] = 0.f; xq[r][i] = 0.f; }
        if (DW && x0 + r < a.W)
          unpack8(*reinterpret_cast<const uint4*>(a.x + ((long)(b * a.H + iy) * a.W + x0 + r) * a.ldx + cg * 8), xq[r]);
      }
      gather_run<M, R, DX, DW>(a.g + (long)b * a.Ho * a.Wo * a.ldg + cg * 8, a.ldg, a.Ho, a.Wo, iy, x0, a.dil, w, acc, xq, dw);
      if (DX) {
        bf16_t* xo = a.out + ((long)(b * a.H + iy) * a.W + x0) * a.ldo + cg * 8;
#pragma unroll
        for (int r = 0; r < R; ++r)
          if (x0 + r < a.W) *reinterpret_cast<uint4*>(xo + (long)r * a.ldo) = pack8(acc[r]);
      }
    }
  if (DW) {
    const int C = a.C;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      // tap k of the forward multiplied x[o s - d + k d]: the gather's tap index IS the forward's
      float* dst = a.ws + ((long)blockIdx.x * 9 + k) * C;
      reduce_rows(dw[k], red, ln, C, [=](int c, double s) { dst[c] = (float)s; });
    }
  }
}

// dw[c][t] (+)= sum over the workgroups' partials ws[blk][t][c], in workgroup order
// (32 results per workgroup, the partials of each dealt over 8 threads: 9 C / 32 workgroups stream the table)
__global__ __launch_bounds__(NT) void dwconv_wsum_kernel(const float* __restrict__ ws, int blocks, int C,
                                                         float* __restrict__ dw, int accumulate) {
  __shared__ float part[8][32];
  const int lo = threadIdx.x & 31, ks = threadIdx.x >> 5;
  const int o = blockIdx.x * 32 + lo;                   // = t * C + c
  float s = 0.f;
  if (o < 9 * C)
    for (int k = ks; k < blocks; k += 8) s += ws[(long)k * 9 * C + o];
  part[ks][lo] = s;
  __syncthreads();
  if (ks == 0 && o < 9 * C) {
#pragma unroll
    for (int k = 1; k < 8; ++k) s += part[k][lo];
    const int tp = o / C, c = o - tp * C;
    float* d = dw + c * 9 + tp;
    *d = accumulate ? *d + s : s;
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// -1: a bad descriptor; -2: a form the kernels are not built for; 0: fine
int check_desc(const ssa_dwconv_desc* d) {
  if (!d || d->B < 1 || d->H < 1 || d->W < 1 || d->C < 8 || d->C % 8) return SSA_EINVAL;
  if (d->ldx < d->C || d->ldy < d->C || d->ldx % 8 || d->ldy % 8) return SSA_EINVAL;
  if (!((d->stride == 1 && d->dil >= 1) || (d->stride == 2 && d->dil == 1))) return SSA_EINVAL;
  if (d->Ho != (d->H - 1) / d->stride + 1 || d->Wo != (d->W - 1) / d->stride + 1) return SSA_EINVAL;
  return SSA_OK;
}

// grid = (workgroups along the runs, channel tiles)
dim3 plan_grid(const ssa_dwconv_desc& d, long runs, int cap) {
  const int VC = d.C >> 3, TW = VC < kTile ? VC : kTile, RP = NT / TW, tiles = (VC + TW - 1) / TW;
  const long want = (runs + RP - 1) / RP, most = cap / tiles > 1 ? cap / tiles : 1;
  return dim3((unsigned)(want > most ? most : want), (unsigned)tiles);
}
dim3 fwd_grid(const ssa_dwconv_desc& d) {
  return plan_grid(d, (long)d.B * d.Ho * ((d.Wo + kRunFwd - 1) / kRunFwd), kFwdBlocks);
}
dim3 bwd_grid(const ssa_dwconv_desc& d) {
  return plan_grid(d, (long)d.B * d.H * ((d.W + kRunBwd - 1) / kRunBwd), kBwdBlocks);
}

template <int S, int DIL>
int launch_bwd(const DwArgs& a, dim3 grid, bool dx, bool dw, hipStream_t s) {
  if (dx && dw) hipLaunchKernelGGL((dwconv_bwd_kernel<S, DIL, true, true>), grid, dim3(NT), 0, s, a);
  else if (dx) hipLaunchKernelGGL((dwconv_bwd_kernel<S, DIL, true, false>), grid, dim3(NT), 0, s, a);
  else hipLaunchKernelGGL((dwconv_bwd_kernel<S, DIL, false, true>), grid, dim3(NT), 0, s, a);
  SSA_LAUNCH_CHECK();
  return SSA_OK;
}

}  // namespace

extern "C" {

int ssa_dwconv3x3(const ssa_dwconv_desc* d, const void* x, const float* w, void* y, double* stats, const float* coef,
                  int relu, void* stream) {
  if (const int rc = check_desc(d)) return rc;
  if (!x || !w || !y || !aligned16(x) || !aligned16(y) || !aligned16(w)) return SSA_EINVAL;      // (w: 16-byte loads too)
  if (stats && coef) return SSA_EUNSUPPORTED;
  DwArgs a = {(const bf16_t*)x, nullptr, w, (bf16_t*)y, stats, coef, nullptr,
              d->B, d->H, d->W, d->C, d->ldx, d->Ho, d->Wo, 0, d->ldy, d->dil, relu ? 1 : 0};
  const dim3 grid = fwd_grid(*d), block(NT);
  hipStream_t s = (hipStream_t)stream;
  if (d->stride == 2) hipLaunchKernelGGL((dwconv_fwd_kernel<2, 1>), grid, block, 0, s, a);
  else if (d->dil == 1) hipLaunchKernelGGL((dwconv_fwd_kernel<1, 1>), grid, block, 0, s, a);
  else if (d->dil == 2) hipLaunchKernelGGL((dwconv_fwd_kernel<1, 2>), grid, block, 0, s, a);
  else if (d->dil == 4) hipLaunchKernelGGL((dwconv_fwd_kernel<1, 4>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((dwconv_fwd_kernel<1, 0>), grid, block, 0, s, a);
  SSA_LAUNCH_CHECK();
  return SSA_OK;
}

int ssa_dwconv3x3_bwd_plan(const ssa_dwconv_desc* d, size_t* ws_bytes) {
  if (const int rc = check_desc(d)) return rc;
  if (!ws_bytes) return SSA_EINVAL;
  *ws_bytes = (size_t)bwd_grid(*d).x * 9 * d->C * sizeof(float);
  return SSA_OK;
}

int ssa_dwconv3x3_bwd(const ssa_dwconv_desc* d, const void* x, const void* dy, int lddy, const float* w, void* dx,
                      int lddx, float* dw, int accumulate, void* ws, void* stream) {
  if (const int rc = check_desc(d)) return rc;
  if (!dy || !w || (!dx && !dw) || lddy < d->C || lddy % 8 || !aligned16(dy) || !aligned16(w)) return SSA_EINVAL;
  if (dx && (lddx < d->C || lddx % 8 || !aligned16(dx))) return SSA_EINVAL;
  if (dw && (!x || !ws || !aligned16(x))) return SSA_EINVAL;
  DwArgs a = {(const bf16_t*)x, (const bf16_t*)dy, w, (bf16_t*)dx, nullptr, nullptr, (float*)ws,
              d->B, d->H, d->W, d->C, d->ldx, d->Ho, d->Wo, lddy, lddx, d->dil, 0};
  const dim3 grid = bwd_grid(*d);
  hipStream_t s = (hipStream_t)stream;
  int rc;
  if (d->stride == 2) rc = launch_bwd<2, 1>(a, grid, dx != nullptr, dw != nullptr, s);
  else if (d->dil == 1) rc = launch_bwd<1, 1>(a, grid, dx != nullptr, dw != nullptr, s);
  else if (d->dil == 2) rc = launch_bwd<1, 2>(a, grid, dx != nullptr, dw != nullptr, s);
  else if (d->dil == 4) rc = launch_bwd<1, 4>(a, grid, dx != nullptr, dw != nullptr, s);
  else rc = launch_bwd<1, 0>(a, grid, dx != nullptr, dw != nullptr, s);
  if (rc) return rc;
  if (dw) {
    hipLaunchKernelGGL(dwconv_wsum_kernel, dim3((9 * d->C + 31) / 32), dim3(NT), 0, s, (const float*)ws, (int)grid.x,
                       d->C, dw, accumulate);
    SSA_LAUNCH_CHECK();
  }
  return SSA_OK;
}

}  // extern "C"
