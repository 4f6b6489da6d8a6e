// Boundary label relaxation (--jointwtborder), "Improving Semantic Segmentation via Video Propagation and Label
// Relaxation":
//   * RelaxedBoundaryLossToTensor   transforms/transforms.py:74-123   (K16)
//   * ImgWtLossSoftNLL              loss/utils.py:150-231             (K16)
// The reference builds a [C+1,H,W] uint8 multi-hot target per sample on the host ((2b+1)^2 scipy shifts) and runs ten
// full-size torch ops and two host round trips per image over it.  Here the target of a pixel is a class SET of two
// 64-bit words (bit c = class c, bit C = the ignore channel), made from the int64 label map that is already on the
// device by a (2b+1)^2 stencil over an LDS tile; the loss is one streaming pass over the logits with the staged
// [256][C] tile of pixel_loss_kernel (loss.hip).  fp32 per pixel, fp64 across pixels; every count is an integer sum.
//
// For the classes of a set  log(max(soft_c, m_c * S)) = log S  with S = sum_{c in set} soft_c  (S >= soft_c in floating
// point too), so the pixel's term is  -q * (sum_{c in set} w_c) * log S  and classes outside the set are never
// evaluated: where the reference forms 0 * log(0) = NaN for an underflowed class outside the set, this stays finite.
// log S is taken as a difference of two log-sum-exps, each about its own maximum.
#include "common.h"
#include "group.h"
#include "../../include/semseg_hip.h"
#include <float.h>

namespace {

constexpr int NT = 256;
constexpr int TW = 32, TH = 8;      // label tile of the stencil kernel: one pixel per thread
constexpr int MAXB = 2;             // cfg.BORDER_WINDOW up to 2: a 5 x 5 window
constexpr int MAXC = 127;           // classes; bit C of the second word is then the ignore channel

struct alignas(16) Set2 { unsigned long long lo, hi; };

// masks of the real classes (everything below bit C)
__device__ __forceinline__ unsigned long long real_lo(int C) { return C >= 64 ? ~0ull : (1ull << C) - 1ull; }
__device__ __forceinline__ unsigned long long real_hi(int C) { return C <= 64 ? 0ull : (1ull << (C - 64)) - 1ull; }
__device__ __forceinline__ void set_bit(Set2& s, int c) {
  if (c < 64) s.lo |= 1ull << c; else s.hi |= 1ull << (c - 64);
}
__device__ __forceinline__ bool has_bit(unsigned long long lo, unsigned long long hi, int c) {
  return ((c < 64 ? lo >> c : hi >> (c - 64)) & 1ull) != 0;
}

// one pixel's set into the workgroup's histogram: bins 0..C the channels, bin C+1 the pixels without a real class
__device__ __forceinline__ void hist_add(unsigned* hist, const Set2& s, int C) {
  unsigned long long lo = s.lo, hi = s.hi;
  while (lo) { atomicAdd(&hist[__builtin_ctzll(lo)], 1u); lo &= lo - 1ull; }
  while (hi) { atomicAdd(&hist[64 + __builtin_ctzll(hi)], 1u); hi &= hi - 1ull; }
  if (((s.lo & real_lo(C)) | (s.hi & real_hi(C))) == 0ull) atomicAdd(&hist[C + 1], 1u);
}
// the workgroup's histogram into the image's int64 counters: one atomic per non-empty bin
__device__ __forceinline__ void hist_flush(const unsigned* hist, int C, int64_t* stats) {
  for (int c = threadIdx.x; c < C + 2; c += NT)
    if (hist[c]) atomicAdd(reinterpret_cast<unsigned long long*>(stats) + c, (unsigned long long)hist[c]);
}

// The counters of the two mask kernels start from zero: cleared by a launch of its own in front of them, on the same
// stream, so that a captured step clears them at every replay.
__global__ __launch_bounds__(NT) void relax_zero_kernel(int64_t* __restrict__ stats, int n) {
  for (int i = threadIdx.x; i < n; i += NT) stats[i] = 0;
}

// Sets from labels.  grid (tiles taken in strides, B).  A workgroup stages the (TH + 2b) x (TW + 2b) class indices of
// a tile and its halo as bytes (0..C; outside the image = C), every thread ORs the (2b+1)^2 bits of its window.
template <typename LT>
__global__ __launch_bounds__(NT) void relax_mask_labels_kernel(const LT* __restrict__ labels, int H, int W, int C,
                                                               int ignore_index, int border, unsigned long long strict_lo,
                                                               unsigned long long strict_hi, Set2* __restrict__ sets,
                                                               int64_t* __restrict__ stats) {
  __shared__ unsigned char lab[(TH + 2 * MAXB) * (TW + 2 * MAXB)];
  __shared__ unsigned hist[MAXC + 2];
  const int b = blockIdx.y;
  const int SW = TW + 2 * border, SH = TH + 2 * border;
  const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
  const LT* img = labels + (long)b * H * W;
  for (int c = threadIdx.x; c < C + 2; c += NT) hist[c] = 0u;
  const int lx = threadIdx.x % TW, ly = threadIdx.x / TW;
  for (int t = blockIdx.x; t < tiles_x * tiles_y; t += gridDim.x) {
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    const int y0 = ty * TH - border, x0 = tx * TW - border;
    __syncthreads();                       // the previous tile's readers are done (and hist is zeroed)
    for (int i = threadIdx.x; i < SH * SW; i += NT) {
      const int r = i / SW, q = i - r * SW;
      const int y = y0 + r, x = x0 + q;
      int v = C;
      if (y >= 0 && y < H && x >= 0 && x < W) {
        const long l = (long)img[(long)y * W + x];
        if (l != ignore_index && l >= 0 && l < C) v = (int)l;
      }
      lab[i] = (unsigned char)v;
    }
    __syncthreads();
    const int y = ty * TH + ly, x = tx * TW + lx;
    if (y < H && x < W) {
      Set2 s = {0ull, 0ull};
      const int own = lab[(ly + border) * SW + lx + border];
      if (has_bit(strict_lo, strict_hi, own)) {
        set_bit(s, own);
      } else {
        for (int dy = 0; dy <= 2 * border; ++dy)
          for (int dx = 0; dx <= 2 * border; ++dx) set_bit(s, lab[(ly + dy) * SW + lx + dx]);
      }
      sets[((long)b * H + y) * W + x] = s;
      hist_add(hist, s, C);
    }
  }
  __syncthreads();
  hist_flush(hist, C, stats + (long)b * (C + 2));
}

// Sets from the reference's multi-hot target uint8 [B][C+1][H][W] (non-zero = set).  grid (chunks in strides, B).
__global__ __launch_bounds__(NT) void relax_mask_multihot_kernel(const unsigned char* __restrict__ mh, long HW, int C,
                                                                 Set2* __restrict__ sets, int64_t* __restrict__ stats) {
  __shared__ unsigned hist[MAXC + 2];
  const int b = blockIdx.y;
  for (int c = threadIdx.x; c < C + 2; c += NT) hist[c] = 0u;
  __syncthreads();
  const unsigned char* img = mh + (long)b * (C + 1) * HW;
  for (long p = (long)blockIdx.x * NT + threadIdx.x; p < HW; p += (long)gridDim.x * NT) {
    Set2 s = {0ull, 0ull};
    for (int c = 0; c <= C; ++c)
      if (img[(long)c * HW + p]) set_bit(s, c);
    sets[(long)b * HW + p] = s;
    hist_add(hist, s, C);
  }
  __syncthreads();
  hist_flush(hist, C, stats + (long)b * (C + 2));
}

// Multi-hot uint8 [B][C+1][H][W] from the sets: a thread takes four consecutive pixels of an image and writes one
// 32-bit word per channel (byte stores where H*W is no multiple of 4 or the output is not 4-byte aligned).
__global__ __launch_bounds__(NT) void relax_multihot_kernel(const Set2* __restrict__ sets, long HW, int C, int words,
                                                            unsigned char* __restrict__ out) {
  const int b = blockIdx.y;
  const long ngroups = (HW + 3) / 4;
  unsigned char* img = out + (long)b * (C + 1) * HW;
  for (long g = (long)blockIdx.x * NT + threadIdx.x; g < ngroups; g += (long)gridDim.x * NT) {
    const long p0 = g * 4;
    const int n = (int)min(4L, HW - p0);
    Set2 s[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = sets[(long)b * HW + (k < n ? p0 + k : p0)];
    for (int c = 0; c <= C; ++c) {
      unsigned v = 0u;
#pragma unroll
      for (int k = 0; k < 4; ++k) v |= (has_bit(s[k].lo, s[k].hi, c) ? 1u : 0u) << (8 * k);
      unsigned char* dst = img + (long)c * HW + p0;
      if (words) {
        *reinterpret_cast<unsigned*>(dst) = v;
      } else {
        for (int k = 0; k < n; ++k) dst[k] = (unsigned char)((v >> (8 * k)) & 0xffu);
      }
    }
  }
}

// calculate_weights in the reference's fp64 (numpy), one rounding to fp32 (torch.Tensor): every product and sum is
// rounded on its own, as numpy's array expression does -- no fused multiply-add.
__global__ __launch_bounds__(128) void relax_weights_kernel(const int64_t* __restrict__ stats, int B, int C,
                                                            double upper_bound, int batch_weights,
                                                            float* __restrict__ w, double* __restrict__ acc) {
#pragma clang fp contract(off)
  for (int i = threadIdx.x; i < B; i += 128) acc[i] = 0.0;
  const int c = threadIdx.x;
  if (c >= C) return;
  int64_t bcnt = 0, btot = 0;
  if (batch_weights)
    for (int i = 0; i < B; ++i) {
      bcnt += stats[(long)i * (C + 2) + c];
      for (int k = 0; k <= C; ++k) btot += stats[(long)i * (C + 2) + k];
    }
  for (int i = 0; i < B; ++i) {
    int64_t cnt = bcnt, tot = btot;
    if (!batch_weights) {
      cnt = stats[(long)i * (C + 2) + c];
      tot = 0;
      for (int k = 0; k <= C; ++k) tot += stats[(long)i * (C + 2) + k];
    }
    const double hist = (double)cnt * 1.0 / (double)tot;
    const double on = (hist != 0.0 ? 1.0 : 0.0) * upper_bound;
    const double scaled = on * (1.0 - hist);
    w[(long)i * C + c] = (float)(scaled + 1.0);
  }
}

// The loss (GRAD = false: per-image fp64 sums into acc) and its backward recomputed from the logits (GRAD = true: the
// scaled gradient into dlogits, dense [P][C]).  grid (256-pixel tiles of an image in strides, B).
template <bool GRAD>
__global__ __launch_bounds__(NT) void relax_nll_kernel(const float* __restrict__ logits, int ld,
                                                       const Set2* __restrict__ sets, const float* __restrict__ w,
                                                       const int64_t* __restrict__ stats, int B, long HW, int C,
                                                       double* __restrict__ acc, const float* __restrict__ upstream,
                                                       float* __restrict__ dlogits) {
  SSA_DYN_LDS(float, tile);  // [NT][C]
  __shared__ float wsh[MAXC + 1];
  __shared__ double red[NT / 64];
  const int img = blockIdx.y;
  for (int c = threadIdx.x; c < C; c += NT) wsh[c] = w[(long)img * C + c];
  const unsigned long long rlo = real_lo(C), rhi = real_hi(C);
  float gscale = 0.f;
  if (GRAD) gscale = (float)((double)upstream[0] / (double)(HW - stats[(long)img * (C + 2) + C + 1] + 1));
  double lsum = 0.0;
  for (long base = (long)blockIdx.x * NT; base < HW; base += (long)gridDim.x * NT) {
    const long npx = min((long)NT, HW - base);
    const long n = npx * C;
    // coalesced stage-in (float4 where the tile starts on 16 bytes)
    if (ld == C) {
      const float* src = logits + ((long)img * HW + base) * C;
      const long n4 = (reinterpret_cast<uintptr_t>(src) & 15u) == 0 ? n >> 2 : 0;
      for (long i = threadIdx.x; i < n4; i += NT)
        reinterpret_cast<float4*>(tile)[i] = reinterpret_cast<const float4*>(src)[i];
      for (long i = n4 * 4 + threadIdx.x; i < n; i += NT) tile[i] = src[i];
    } else {
      const float* src = logits + ((long)img * HW + base) * ld;
      for (long i = threadIdx.x; i < n; i += NT) tile[i] = src[(i / C) * ld + i % C];
    }
    __syncthreads();
    if (threadIdx.x < npx) {
      float* x = tile + threadIdx.x * C;
      const long p = base + threadIdx.x;
      const Set2 own = sets[(long)img * HW + p];
      const unsigned long long lo = own.lo & rlo, hi = own.hi & rhi;
      if ((lo | hi) == 0ull) {
        if (GRAD)
          for (int c = 0; c < C; ++c) x[c] = 0.f;
      } else {
        // q = sum over the batch of 1 / border weight (loss/utils.py:196,228: the whole [B,H,W] tensor broadcasts)
        float q = 0.f;
        for (int b = 0; b < B; ++b) {
          const Set2 s = sets[(long)b * HW + p];
          const int bw = __builtin_popcountll(s.lo & rlo) + __builtin_popcountll(s.hi & rhi);
          q += 1.f / (float)(bw > 0 ? bw : 1);
        }
        float mx = -FLT_MAX;
        for (int c = 0; c < C; ++c) mx = fmaxf(mx, x[c]);
        float se = 0.f;
        for (int c = 0; c < C; ++c) se += __expf(x[c] - mx);
        float mxm = -FLT_MAX, ws = 0.f;
        for (unsigned long long m = lo; m; m &= m - 1ull) { const int c = __builtin_ctzll(m); mxm = fmaxf(mxm, x[c]); ws += wsh[c]; }
        for (unsigned long long m = hi; m; m &= m - 1ull) { const int c = 64 + __builtin_ctzll(m); mxm = fmaxf(mxm, x[c]); ws += wsh[c]; }
        float sm = 0.f;
        for (unsigned long long m = lo; m; m &= m - 1ull) sm += __expf(x[__builtin_ctzll(m)] - mxm);
        for (unsigned long long m = hi; m; m &= m - 1ull) sm += __expf(x[64 + __builtin_ctzll(m)] - mxm);
        const float lse = mx + __logf(se), lsm = mxm + __logf(sm);
        if (!GRAD) {
          lsum += (double)(-q * ws * (lsm - lse));
        } else {
          // d(-log S)/dz_k = soft_k - [k in set] soft_k / S,  soft_k / S = exp(z_k - lsm)
          const float coef = q * ws * gscale;
          for (int c = 0; c < C; ++c) {
            const float v = x[c];
            const float in = has_bit(lo, hi, c) ? __expf(v - lsm) : 0.f;
            x[c] = coef * (__expf(v - lse) - in);
          }
        }
      }
    }
    if (GRAD) {
      __syncthreads();
      float* dst = dlogits + ((long)img * HW + base) * C;  // gradient buffer is dense [P, C]
      const long n4 = (reinterpret_cast<uintptr_t>(dst) & 15u) == 0 ? n >> 2 : 0;
      for (long i = threadIdx.x; i < n4; i += NT)
        reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(tile)[i];
      for (long i = n4 * 4 + threadIdx.x; i < n; i += NT) dst[i] = tile[i];
    }
    __syncthreads();
  }
  if (!GRAD) {
    lsum = wave_sum_d(lsum);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = lsum;
    __syncthreads();
    if (threadIdx.x == 0) {
      double s = 0.0;
      for (int i = 0; i < NT / 64; ++i) s += red[i];
      atomicAdd(&acc[img], s);
    }
  }
}

__global__ void relax_finalize_kernel(const double* __restrict__ acc, const int64_t* __restrict__ stats, int B, long HW,
                                      int C, float* __restrict__ loss) {
  double s = 0.0;
  for (int i = 0; i < B; ++i) s += acc[i] / (double)(HW - stats[(long)i * (C + 2) + C + 1] + 1);
  loss[0] = (float)s;
}

inline int strided_grid(long items, int B, int cap) {
  long g = items, per = cap / B;
  if (per < 1) per = 1;
  if (g > per) g = per;
  if (g < 1) g = 1;
  return (int)g;
}

inline int shape_rc(int B, int H, int W, int C) {
  if (B <= 0 || H <= 0 || W <= 0 || B > 65535) return SSA_EINVAL;
  if (C < 1 || C > MAXC) return SSA_EUNSUPPORTED;
  return SSA_OK;
}

template <bool GRAD>
int launch_nll(const float* logits, int ld, const unsigned long long* sets, const float* w, const int64_t* stats, int B,
               int H, int W, int C, double* acc, const float* upstream, float* dlogits, hipStream_t s) {
  const size_t lds = (size_t)NT * C * sizeof(float);
  {   // the [NT][C] fp32 tile exceeds the default 64 KB of dynamic LDS from 65 classes (Mapillary) on
    static ssa::LdsLimit lds_limit;         // per device (group.h)
    if (int rc = ssa::raise_lds_limit((const void*)relax_nll_kernel<GRAD>, lds, 64 * 1024, &lds_limit)) return rc;
  }
  const long HW = (long)H * W;
  hipLaunchKernelGGL(relax_nll_kernel<GRAD>, dim3(strided_grid((HW + NT - 1) / NT, B, 2048), B), dim3(NT), lds, s, logits,
                     ld, reinterpret_cast<const Set2*>(sets), w, stats, B, HW, C, acc, upstream, dlogits);
  SSA_LAUNCH_CHECK();
  return SSA_OK;
}

}  // namespace

extern "C" {

int ssa_relax_mask_labels(const void* labels, int label_u8, int B, int H, int W, int C, int ignore_index, int border,
                          unsigned long long strict_lo, unsigned long long strict_hi, unsigned long long* sets,
                          int64_t* stats, void* stream) {
  if (!labels || !sets || !stats) return SSA_EINVAL;
  if (int rc = shape_rc(B, H, W, C)) return rc;
  if (border < 0 || border > MAXB) return SSA_EUNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(sets) & 15u) != 0) return SSA_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(relax_zero_kernel, dim3(1), dim3(NT), 0, s, stats, B * (C + 2));
  SSA_LAUNCH_CHECK();
  // the ignore channel is never strict: a pixel outside the classes keeps its window
  strict_lo &= C >= 64 ? ~0ull : (1ull << C) - 1ull;
  strict_hi &= C <= 64 ? 0ull : (1ull << (C - 64)) - 1ull;
  const long tiles = (long)((W + TW - 1) / TW) * ((H + TH - 1) / TH);
  const dim3 grid(strided_grid(tiles, B, 1024), B);
  if (label_u8)
    hipLaunchKernelGGL(relax_mask_labels_kernel<unsigned char>, grid, dim3(NT), 0, s, (const unsigned char*)labels, H, W, C,
                       ignore_index, border, strict_lo, strict_hi, reinterpret_cast<Set2*>(sets), stats);
  else
    hipLaunchKernelGGL(relax_mask_labels_kernel<int64_t>, grid, dim3(NT), 0, s, (const int64_t*)labels, H, W, C,
                       ignore_index, border, strict_lo, strict_hi, reinterpret_cast<Set2*>(sets), stats);
  SSA_LAUNCH_CHECK();
  return SSA_OK;
}

int ssa_relax_mask_multihot(const unsigned char* multihot, int B, int H, int W, int C, unsigned long long* sets,
                            int64_t* stats, void* stream) {
  if (!multihot || !sets || !stats) return SSA_EINVAL;
  if (int rc = shape_rc(B, H, W, C)) return rc;
  if ((reinterpret_cast<uintptr_t>(sets) & 15u) != 0) return SSA_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(relax_zero_kernel, dim3(1), dim3(NT), 0, s, stats, B * (C + 2));
  SSA_LAUNCH_CHECK();
  const long HW = (long)H * W;
  hipLaunchKernelGGL(relax_mask_multihot_kernel, dim3(strided_grid((HW + NT - 1) / NT, B, 1024), B), dim3(NT), 0, s,
                     multihot, HW, C, reinterpret_cast<Set2*>(sets), stats);
  SSA_LAUNCH_CHECK();
  return SSA_OK;
}

int ssa_relax_multihot(const unsigned long long* sets, int B, int H, int W, int C, unsigned char* out, void* stream) {
  if (!sets || !out) return SSA_EINVAL;
  if (int rc = shape_rc(B, H, W, C)) return rc;
  if ((reinterpret_cast<uintptr_t>(sets) & 15u) != 0) return SSA_EINVAL;
  const long HW = (long)H * W;
  const int words = (HW % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 3u) == 0) ? 1 : 0;
  hipLaunchKernelGGL(relax_multihot_kernel, dim3(strided_grid(((HW + 3) / 4 + NT - 1) / NT, B, 4096), B), dim3(NT), 0,
                     (hipStream_t)stream, reinterpret_cast<const Set2*>(sets), HW, C, words, out);
  SSA_LAUNCH_CHECK();
  return SSA_OK;
}

int ssa_relax_weights(const int64_t* stats, int B, int C, double upper_bound, int batch_weights, float* w, double* acc,
                      void* stream) {
  if (!stats || !w || !acc) return SSA_EINVAL;
  if (int rc = shape_rc(B, 1, 1, C)) return rc;
  hipLaunchKernelGGL(relax_weights_kernel, dim3(1), dim3(128), 0, (hipStream_t)stream, stats, B, C, upper_bound,
                     batch_weights ? 1 : 0, w, acc);
  SSA_LAUNCH_CHECK();
  return SSA_OK;
}

int ssa_relax_nll_fwd(const float* logits, int ld, const unsigned long long* sets, const float* w, int B, int H, int W,
                      int C, double* acc, void* stream) {
  if (!logits || !sets || !w || !acc) return SSA_EINVAL;
  if (int rc = shape_rc(B, H, W, C)) return rc;
  if (ld < C || (reinterpret_cast<uintptr_t>(sets) & 15u) != 0) return SSA_EINVAL;
  return launch_nll<false>(logits, ld, sets, w, nullptr, B, H, W, C, acc, nullptr, nullptr, (hipStream_t)stream);
}

int ssa_relax_nll_finalize(const double* acc, const int64_t* stats, int B, int H, int W, int C, float* loss,
                           void* stream) {
  if (!acc || !stats || !loss) return SSA_EINVAL;
  if (int rc = shape_rc(B, H, W, C)) return rc;
  hipLaunchKernelGGL(relax_finalize_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, acc, stats, B, (long)H * W, C, loss);
  SSA_LAUNCH_CHECK();
  return SSA_OK;
}

int ssa_relax_nll_bwd(const float* logits, int ld, const unsigned long long* sets, const float* w, const int64_t* stats,
                      int B, int H, int W, int C, const float* upstream, float* dlogits, void* stream) {
  if (!logits || !sets || !w || !stats || !upstream || !dlogits) return SSA_EINVAL;
  if (int rc = shape_rc(B, H, W, C)) return rc;
  if (ld < C || (reinterpret_cast<uintptr_t>(sets) & 15u) != 0) return SSA_EINVAL;
  return launch_nll<true>(logits, ld, sets, w, stats, B, H, W, C, nullptr, upstream, dlogits, (hipStream_t)stream);
}

}  // extern "C"
