// Adam, AMSGrad and RAdam over every parameter tensor of the net in a handful of launches (train.py:509
// `optim.step()` on the torch.optim.Adam of loss/optimizer.py:55-59 or the RAdam of loss/optimizer.py:60-63,
// loss/radam.py:29-107), the sibling of sgd_momentum_kernel (optim.hip).
//
// HBM-bound streaming update: per element read p, g, m, v and write p, m, v (28 B; AMSGrad also reads and writes
// the running maximum of v: 36 B), one pass.  Up to 56 tensors ride in one launch: their pointers and chunk prefix
// sums are KERNEL ARGUMENTS (3.4 KB of the 4 KB limit), so nothing is uploaded and a captured hipGraph holds the
// whole update.
//
// What depends on the step count t lives in a 16-byte DEVICE record per parameter,  {t, rectified, c1, c2}:
//   ssa_adam_advance   one thread per parameter of this step's list: t += 1, then in double precision
//                      Adam / AMSGrad  c1 = 1 / (1 - beta1^t)          c2 = 1 / sqrt(1 - beta2^t)
//                      RAdam           N_sma = N_max - 2 t beta2^t / (1 - beta2^t),  rectified = N_sma >= 5,
//                                      c1 = step_size / lr of loss/radam.py:80-90
//   ssa_adam_step      reads the record: no pow() per element, nothing computed on the host, so a replayed graph
//                      counts its own steps and takes RAdam's branch on the device.
// With a loss-scaling record (optim.hip) both do NOTHING when found_inf is set -- a skipped step leaves t, m, v,
// vmax and p untouched, as apex does -- and the update multiplies every gradient by 1 / scale.
#include "common.h"
#include "../../include/semseg_hip.h"
#include <math.h>

namespace {

constexpr int kTensors = 56;          // tensors per launch
constexpr int kThreads = 256;
constexpr int kChunk = kThreads * 16; // elements per workgroup
constexpr int kRecs = 448;            // records per launch of the advance kernel

enum { kAdam = 0, kAmsgrad = 1, kRAdam = 2 };

struct AdamRec {
  int step;                           // t: updates this parameter has taken
  int rect;                           // RAdam: the variance is tractable (N_sma >= 5); Adam: 1
  float c1;                           // factor of lr in the step size
  float c2;                           // Adam: 1 / sqrt(1 - beta2^t)
};

struct AdamBatch {
  float* p[kTensors];
  const float* g[kTensors];
  float* m[kTensors];
  float* v[kTensors];
  float* vmax[kTensors];              // AMSGrad only
  const AdamRec* rec[kTensors];
  long numel[kTensors];
  int chunk_start[kTensors + 1];      // prefix sum of ceil(numel / kChunk)
  int n;
};
static_assert(sizeof(AdamBatch) <= 3456, "the batch and the hyper-parameters must fit the kernel arguments");

struct AdamHyper {
  float lr;
  const float* lr_dev;                // when set, overrides lr
  float beta1, one_minus_beta1, beta2, one_minus_beta2, eps, weight_decay;
  const float* amp;                   // loss-scaling record {scale, found_inf, clean steps, 1 / scale} or null
};

struct RecBatch {
  AdamRec* rec[kRecs];
  int n;
};

// per-step scalars of one parameter, read from its record once per workgroup
struct StepScalars {
  float step_size, c2, decay;
  bool rect;
};

// Adam / AMSGrad: torch.optim.Adam's single-tensor update with L2 weight decay
//   g += wd p;  m += (1 - b1)(g - m);  v = b2 v + (1 - b2) g g;  p -= lr c1 * m / (sqrt(v | vmax) c2 + eps)
// RAdam: loss/radam.py:63-103 as written -- v, then m; the decay scales p and stays out of the gradient
//   p += -wd lr p;  p -= lr c1 * (rectified ? m / (sqrt(v) + eps) : m)
template <int MODE>
__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, float& vmax, const AdamHyper& hp,
                                            const StepScalars& s) {
  if (MODE == kRAdam) {
    v = __fmaf_rn(hp.beta2, v, __fmul_rn(__fmul_rn(hp.one_minus_beta2, g), g));
    m = __fmaf_rn(hp.beta1, m, __fmul_rn(hp.one_minus_beta1, g));
    if (hp.weight_decay != 0.f) p = __fmaf_rn(s.decay, p, p);
    const float d = s.rect ? m / (sqrtf(v) + hp.eps) : m;
    p = __fmaf_rn(-s.step_size, d, p);
  } else {
    if (hp.weight_decay != 0.f) g = __fmaf_rn(hp.weight_decay, p, g);
    m = __fmaf_rn(hp.one_minus_beta1, g - m, m);
    v = __fmaf_rn(hp.beta2, v, __fmul_rn(__fmul_rn(hp.one_minus_beta2, g), g));
    float vd = v;
    if (MODE == kAmsgrad) vd = vmax = fmaxf(vmax, v);
    p = __fmaf_rn(-s.step_size, m / __fmaf_rn(sqrtf(vd), s.c2, hp.eps), p);
  }
}

template <int MODE>
__global__ __launch_bounds__(kThreads) void adam_kernel(const AdamBatch tb, const AdamHyper hp) {
  // which tensor does this workgroup's chunk belong to
  int lo = 0, hi = tb.n;
  const int blk = blockIdx.x;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tb.chunk_start[mid] <= blk) lo = mid; else hi = mid;
  }
  const int t = lo;
  float* __restrict__ p = tb.p[t];
  const float* __restrict__ g = tb.g[t];
  float* __restrict__ m = tb.m[t];
  float* __restrict__ v = tb.v[t];
  float* __restrict__ vmax = MODE == kAmsgrad ? tb.vmax[t] : nullptr;
  const long n = tb.numel[t];
  const long base = (long)(blk - tb.chunk_start[t]) * kChunk;
  const long end = base + kChunk < n ? base + kChunk : n;
  float gs = 1.f;                     // gradient un-scaling (fp16 training)
  if (hp.amp) {
    if (hp.amp[1] != 0.f) return;     // an overflowed step is skipped: parameters and moments stay
    gs = hp.amp[3];
  }
  const float lr = hp.lr_dev ? *hp.lr_dev : hp.lr;
  const AdamRec rec = *tb.rec[t];
  StepScalars s;
  s.step_size = __fmul_rn(lr, rec.c1);
  s.c2 = rec.c2;
  s.decay = -__fmul_rn(hp.weight_decay, lr);
  s.rect = rec.rect != 0;
  const bool vec = ((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v) | ((uintptr_t)vmax)) & 15) == 0;
  if (vec) {
    const long vend = base + ((end - base) & ~3L);
    for (long i = base + threadIdx.x * 4L; i < vend; i += kThreads * 4L) {
      float4 pv = *(const float4*)(p + i);
      float4 gv = *(const float4*)(g + i);
      float4 mv = *(const float4*)(m + i);
      float4 vv = *(const float4*)(v + i);
      float4 xv = MODE == kAmsgrad ? *(const float4*)(vmax + i) : make_float4(0.f, 0.f, 0.f, 0.f);
      if (hp.amp) { gv.x *= gs; gv.y *= gs; gv.z *= gs; gv.w *= gs; }
      adam_update<MODE>(pv.x, gv.x, mv.x, vv.x, xv.x, hp, s);
      adam_update<MODE>(pv.y, gv.y, mv.y, vv.y, xv.y, hp, s);
      adam_update<MODE>(pv.z, gv.z, mv.z, vv.z, xv.z, hp, s);
      adam_update<MODE>(pv.w, gv.w, mv.w, vv.w, xv.w, hp, s);
      *(float4*)(p + i) = pv;
      *(float4*)(m + i) = mv;
      *(float4*)(v + i) = vv;
      if (MODE == kAmsgrad) *(float4*)(vmax + i) = xv;
    }
    for (long i = vend + threadIdx.x; i < end; i += kThreads) {
      float pv = p[i], mv = m[i], vv = v[i], xv = MODE == kAmsgrad ? vmax[i] : 0.f;
      adam_update<MODE>(pv, hp.amp ? g[i] * gs : g[i], mv, vv, xv, hp, s);
      p[i] = pv; m[i] = mv; v[i] = vv;
      if (MODE == kAmsgrad) vmax[i] = xv;
    }
  } else {
    for (long i = base + threadIdx.x; i < end; i += kThreads) {
      float pv = p[i], mv = m[i], vv = v[i], xv = MODE == kAmsgrad ? vmax[i] : 0.f;
      adam_update<MODE>(pv, hp.amp ? g[i] * gs : g[i], mv, vv, xv, hp, s);
      p[i] = pv; m[i] = mv; v[i] = vv;
      if (MODE == kAmsgrad) vmax[i] = xv;
    }
  }
}

// one thread per parameter: t += 1 and the factors that depend on t, in double, rounded once
__global__ __launch_bounds__(64) void adam_advance_kernel(const RecBatch rb, int radam, double beta1, double beta2,
                                                          const float* __restrict__ amp) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= rb.n) return;
  if (amp && amp[1] != 0.f) return;   // a skipped step does not count
  AdamRec r = *rb.rec[i];
  r.step += 1;
  const double t = (double)r.step;
  const double bc1 = 1.0 - pow(beta1, t);
  const double beta2_t = pow(beta2, t);
  if (radam) {
    const double n_max = 2.0 / (1.0 - beta2) - 1.0;
    const double n_sma = n_max - 2.0 * t * beta2_t / (1.0 - beta2_t);
    r.rect = n_sma >= 5.0;
    r.c1 = (float)(r.rect ? sqrt((1.0 - beta2_t) * (n_sma - 4.0) / (n_max - 4.0) * (n_sma - 2.0) / n_sma * n_max /
                                 (n_max - 2.0)) / bc1
                          : 1.0 / bc1);
    r.c2 = 1.f;
  } else {
    r.rect = 1;
    r.c1 = (float)(1.0 / bc1);
    r.c2 = (float)(1.0 / sqrt(1.0 - beta2_t));
  }
  *rb.rec[i] = r;
}

bool valid_betas(int mode, double beta1, double beta2) {
  return mode >= kAdam && mode <= kRAdam && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0;
}

}  // namespace

extern "C" int ssa_adam_advance(void* const* recs, int n_tensors, int mode, double beta1, double beta2,
                                const float* amp_state, void* stream) {
  if (n_tensors < 0 || (n_tensors > 0 && !recs) || !valid_betas(mode, beta1, beta2)) return SSA_EINVAL;
  for (int i = 0; i < n_tensors; ++i)
    if (!recs[i] || (((uintptr_t)recs[i]) & 15)) return SSA_EINVAL;
  for (int i = 0; i < n_tensors; i += kRecs) {
    RecBatch rb;
    rb.n = n_tensors - i < kRecs ? n_tensors - i : kRecs;
    for (int k = 0; k < rb.n; ++k) rb.rec[k] = (AdamRec*)recs[i + k];
    hipLaunchKernelGGL(adam_advance_kernel, dim3((rb.n + 63) / 64), dim3(64), 0, (hipStream_t)stream, rb,
                       mode == kRAdam ? 1 : 0, beta1, beta2, amp_state);
    SSA_LAUNCH_CHECK();
  }
  return SSA_OK;
}

extern "C" int ssa_adam_step(void* const* params, const void* const* grads, void* const* exp_avg,
                             void* const* exp_avg_sq, void* const* max_exp_avg_sq, const void* const* recs,
                             const int64_t* numel, int n_tensors, int mode, float lr, const float* lr_dev,
                             double beta1, double beta2, float eps, float weight_decay, const float* amp_state,
                             void* stream) {
  if (n_tensors < 0 || !valid_betas(mode, beta1, beta2) || !(eps >= 0.f) || !(weight_decay >= 0.f)) return SSA_EINVAL;
  if (n_tensors > 0 && (!params || !grads || !exp_avg || !exp_avg_sq || !recs || !numel)) return SSA_EINVAL;
  if (n_tensors > 0 && mode == kAmsgrad && !max_exp_avg_sq) return SSA_EINVAL;
  AdamHyper hp{lr, lr_dev, (float)beta1, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), eps, weight_decay,
               amp_state};
  int i = 0;
  while (i < n_tensors) {
    AdamBatch tb;
    tb.n = 0;
    tb.chunk_start[0] = 0;
    // at most kTensors tensors and 2^20 chunks (4 G elements) per launch
    while (i < n_tensors && tb.n < kTensors && tb.chunk_start[tb.n] < (1 << 20)) {
      const int64_t n = numel[i];
      if (n < 0 || !params[i] || !grads[i] || !exp_avg[i] || !exp_avg_sq[i] || !recs[i] ||
          (((uintptr_t)recs[i]) & 15) || (mode == kAmsgrad && !max_exp_avg_sq[i]))
        return SSA_EINVAL;
      if (n == 0) { ++i; continue; }
      const int64_t chunks = (n + kChunk - 1) / kChunk;
      if (chunks > (1 << 30)) return SSA_EUNSUPPORTED;
      tb.p[tb.n] = (float*)params[i];
      tb.g[tb.n] = (const float*)grads[i];
      tb.m[tb.n] = (float*)exp_avg[i];
      tb.v[tb.n] = (float*)exp_avg_sq[i];
      tb.vmax[tb.n] = mode == kAmsgrad ? (float*)max_exp_avg_sq[i] : nullptr;
      tb.rec[tb.n] = (const AdamRec*)recs[i];
      tb.numel[tb.n] = n;
      tb.chunk_start[tb.n + 1] = tb.chunk_start[tb.n] + (int)chunks;
      ++tb.n;
      ++i;
    }
    if (tb.n == 0) continue;
    const dim3 grid(tb.chunk_start[tb.n]), block(kThreads);
    if (mode == kAdam) hipLaunchKernelGGL(adam_kernel<kAdam>, grid, block, 0, (hipStream_t)stream, tb, hp);
    else if (mode == kAmsgrad) hipLaunchKernelGGL(adam_kernel<kAmsgrad>, grid, block, 0, (hipStream_t)stream, tb, hp);
    else hipLaunchKernelGGL(adam_kernel<kRAdam>, grid, block, 0, (hipStream_t)stream, tb, hp);
    SSA_LAUNCH_CHECK();
  }
  return SSA_OK;
}
