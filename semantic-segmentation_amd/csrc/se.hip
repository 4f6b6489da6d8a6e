// Squeeze-and-excitation gate of the SE-ResNeXt bottleneck on NHWC 16-bit activations (gfx950):
//   z = relu(se_module(y) + residual),  se_module(y) = y * sigmoid(fc2(relu(fc1(avg_pool(y)))))   network/SEresnext.py:84-91, 115-116
// fc1 / fc2 are 1x1 convs with bias on the [B, C] channel means: the gate reads the fp32 parameters directly (their own
// [C/r][C] and [C][C/r] storage) and all of its arithmetic is fp32.
//
// forward   squeeze: per-(image, channel) sums by (image, channel tile, pixel split) workgroups -- enough splits to fill
//           the chip whatever B and C are -- as fp32 partials in `ws`, added up in split order by a small launch
//           (mean = sum / HW); gate: h = relu(W1 mean + b1), s = sigmoid(W2 h + b2), one wave per output;
//           apply: z = round16(relu(fma(s[b,c], y, r))), one streaming pass.
// backward  two passes over dz, because g depends on the complete ds:
//           reduce: ds[b,c] = sum_p m dz y, m = (z > 0), with the squeeze's partial scheme;
//           gate backward (three tiny launches): a2 = ds s (1 - s); db2, dW2 = sum_b a2 h; a1 = (W2^T a2) (h > 0); db1,
//           dW1 = sum_b a1 mean; g = (W1^T a1) / HW;
//           apply backward: dy = round16(fma(s, m dz, g[b,c])), dr = round16(m dz).
// Every sum has a fixed order (no atomics): a result does not depend on scheduling.
#include "common.h"
#include "../../include/semseg_hip.h"

namespace {

constexpr int NT = 256;
constexpr int kTile = 32;          // channel groups (512 bytes of a pixel) per workgroup of the reduce passes
constexpr int kReduceBlocks = 512; // workgroups a reduce pass aims at (two per CU); past it a thread walks more pixels
constexpr int kMaxCr = 1024;

struct Plan { int TW, RP, tiles, nsplit; };

// (image, channel tile, split) decomposition of a per-(image, channel) reduce over HW pixels
Plan plan_reduce(int B, long HW, int C) {
  Plan p;
  const int VC = C >> 3;
  p.TW = VC < kTile ? VC : kTile;
  p.RP = NT / p.TW;
  p.tiles = (VC + p.TW - 1) / p.TW;
  const long want = kReduceBlocks / ((long)B * p.tiles) > 1 ? kReduceBlocks / ((long)B * p.tiles) : 1;
  const long most = (HW + p.RP - 1) / p.RP;
  p.nsplit = (int)(want < most ? want : most);
  return p;
}

// MODE 0: v = y (the squeeze).  MODE 1: v = m dz y, m = (z > 0) with relu, else 1 (the backward reduce).
// part[(b * nsplit + split) * C + c] = sum over the split's pixels, rows of the workgroup added in row order
template <int MODE>
__global__ __launch_bounds__(NT) void se_partial_kernel(const bf16_t* __restrict__ y, int ldy, const bf16_t* __restrict__ dz,
                                                        int lddz, const bf16_t* __restrict__ z, int ldz, long HW, int C,
                                                        int relu, float* __restrict__ part) {
  __shared__ float red[NT * 9];
  const int VC = C >> 3, t = threadIdx.x;
  const int TW = VC < kTile ? VC : kTile, RP = NT / TW;
  const int pr = t / TW, g = blockIdx.y * TW + t % TW, b = blockIdx.z, split = blockIdx.x, nsplit = gridDim.x;
  const bool active = pr < RP && g < VC;
  float acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.f;
  if (active)
    for (long p = (long)split * RP + pr; p < HW; p += (long)nsplit * RP) {
      const long q = (long)b * HW + p;
      float f[8];
      unpack8(*reinterpret_cast<const uint4*>(y + q * ldy + g * 8), f);
      if (MODE == 1) {
        float d[8], m[8];
        unpack8(*reinterpret_cast<const uint4*>(dz + q * lddz + g * 8), d);
        if (relu) {
          unpack8(*reinterpret_cast<const uint4*>(z + q * ldz + g * 8), m);
#pragma unroll
          for (int i = 0; i < 8; ++i) d[i] = m[i] > 0.f ? d[i] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) f[i] *= d[i];
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] += f[i];
    }
#pragma unroll
  for (int i = 0; i < 8; ++i) red[t * 9 + i] = acc[i];
  __syncthreads();
  if (t < TW * 8) {
    const int gg = t >> 3, i = t & 7;
    const int c = (blockIdx.y * TW + gg) * 8 + i;
    if (c < C) {
      double s = 0.0;
      for (int p = 0; p < RP; ++p) s += (double)red[(p * TW + gg) * 9 + i];
      part[((long)b * nsplit + split) * C + c] = (float)s;
    }
  }
}

// out[b][c] = (sum over the splits' partials, in split order within each of 8 interleaved lanes, lanes in order) / div
__global__ __launch_bounds__(NT) void se_finish_kernel(const float* __restrict__ part, int nsplit, int C, float div,
                                                       float* __restrict__ out) {
  __shared__ float sh[8][32];
  const int lo = threadIdx.x & 31, ks = threadIdx.x >> 5, b = blockIdx.y;
  const int c = blockIdx.x * 32 + lo;
  float s = 0.f;
  if (c < C)
    for (int k = ks; k < nsplit; k += 8) s += part[((long)b * nsplit + k) * C + c];
  sh[ks][lo] = s;
  __syncthreads();
  if (ks == 0 && c < C) {
#pragma unroll
    for (int k = 1; k < 8; ++k) s += sh[k][lo];
    out[(long)b * C + c] = s / div;
  }
}

// out[b][o] = act(bias[o] + sum_i w[o][i] in[b][i]): one wave per output (lanes stride the inputs, wave_sum);
// ACT 0: ReLU (fc1), 1: sigmoid (fc2, the formula of ssa_sigmoid_fwd)
template <int ACT>
__global__ __launch_bounds__(NT) void se_fc_kernel(const float* __restrict__ w, const float* __restrict__ bias,
                                                   const float* __restrict__ in, int nin, int nout, float* __restrict__ out) {
  const int lane = threadIdx.x & 63, o = blockIdx.x * (NT / 64) + (threadIdx.x >> 6), b = blockIdx.y;
  if (o >= nout) return;                                   // (wave-uniform)
  float acc = 0.f;
  for (int i = lane; i < nin; i += 64) acc += w[(long)o * nin + i] * in[(long)b * nin + i];
  acc = wave_sum(acc);
  if (lane == 0) {
    const float v = acc + bias[o];
    out[(long)b * nout + o] = ACT == 0 ? fmaxf(v, 0.f) : 1.f / (1.f + __expf(-v));
  }
}

template <bool RES>
__global__ __launch_bounds__(NT) void se_apply_kernel(const bf16_t* __restrict__ y, int ldy, const bf16_t* __restrict__ r,
                                                      int ldr, const float* __restrict__ s, bf16_t* __restrict__ z, int ldz,
                                                      long n, long HW, int C, int relu) {
  const int VC = C >> 3;
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < n; i += (long)gridDim.x * NT) {
    const int cg = (int)(i % VC);
    const long q = i / VC;
    const float* sp = s + (q / HW) * C + cg * 8;
    float f[8], a[8];
    unpack8(*reinterpret_cast<const uint4*>(y + q * ldy + cg * 8), f);
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = 0.f;
    if (RES) unpack8(*reinterpret_cast<const uint4*>(r + q * ldr + cg * 8), a);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      f[j] = fmaf(sp[j], f[j], a[j]);
      if (relu) f[j] = fmaxf(f[j], 0.f);
    }
    *reinterpret_cast<uint4*>(z + q * ldz + cg * 8) = pack8(f);
  }
}

template <bool RES>
__global__ __launch_bounds__(NT) void se_apply_bwd_kernel(const bf16_t* __restrict__ dz, int lddz, const bf16_t* __restrict__ z,
                                                          int ldz, const float* __restrict__ s, const float* __restrict__ g,
                                                          bf16_t* __restrict__ dy, int lddy, bf16_t* __restrict__ dr, int lddr,
                                                          long n, long HW, int C, int relu) {
  const int VC = C >> 3;
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < n; i += (long)gridDim.x * NT) {
    const int cg = (int)(i % VC);
    const long q = i / VC;
    const long bc = (q / HW) * C + cg * 8;
    float d[8], m[8];
    unpack8(*reinterpret_cast<const uint4*>(dz + q * lddz + cg * 8), d);
    if (relu) {
      unpack8(*reinterpret_cast<const uint4*>(z + q * ldz + cg * 8), m);
#pragma unroll
      for (int j = 0; j < 8; ++j) d[j] = m[j] > 0.f ? d[j] : 0.f;
    }
    if (RES) *reinterpret_cast<uint4*>(dr + q * lddr + cg * 8) = pack8(d);
#pragma unroll
    for (int j = 0; j < 8; ++j) d[j] = fmaf(s[bc + j], d[j], g[bc + j]);
    *reinterpret_cast<uint4*>(dy + q * lddy + cg * 8) = pack8(d);
  }
}

// one wave per channel c: a2[b][c] = ds s (1 - s); db2[c] (+)= sum_b a2; dW2[c][j] (+)= sum_b a2[b][c] h[b][j]
__global__ __launch_bounds__(NT) void se_gate_bwd2_kernel(const float* __restrict__ ds, const float* __restrict__ s,
                                                          const float* __restrict__ h, int B, int C, int Cr,
                                                          float* __restrict__ a2, float* __restrict__ dw2,
                                                          float* __restrict__ db2, int accumulate) {
  const int lane = threadIdx.x & 63, c = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
  if (c >= C) return;
  for (int j = lane; j < Cr; j += 64) {
    float acc = 0.f;
    for (int b = 0; b < B; ++b) {
      const float sv = s[(long)b * C + c];
      acc += ds[(long)b * C + c] * (sv * (1.f - sv)) * h[(long)b * Cr + j];
    }
    float* d = dw2 + (long)c * Cr + j;
    *d = accumulate ? *d + acc : acc;
  }
  if (lane == 0) {
    float acc = 0.f;
    for (int b = 0; b < B; ++b) {
      const float sv = s[(long)b * C + c];
      const float v = ds[(long)b * C + c] * (sv * (1.f - sv));
      a2[(long)b * C + c] = v;
      acc += v;
    }
    db2[c] = accumulate ? db2[c] + acc : acc;
  }
}

// one workgroup per hidden unit j: a1[b][j] = (sum_c W2[c][j] a2[b][c]) (h[b][j] > 0); db1[j] (+)= sum_b a1
__global__ __launch_bounds__(NT) void se_gate_bwd1_kernel(const float* __restrict__ a2, const float* __restrict__ w2,
                                                          const float* __restrict__ h, int B, int C, int Cr,
                                                          float* __restrict__ a1, float* __restrict__ db1, int accumulate) {
  __shared__ float sh[NT / 64];
  const int j = blockIdx.x, t = threadIdx.x;
  float sum_b = 0.f;
  for (int b = 0; b < B; ++b) {
    float acc = 0.f;
    for (int c = t; c < C; c += NT) acc += w2[(long)c * Cr + j] * a2[(long)b * C + c];
    acc = wave_sum(acc);
    __syncthreads();
    if ((t & 63) == 0) sh[t >> 6] = acc;
    __syncthreads();
    if (t == 0) {
      const float dh = (sh[0] + sh[1]) + (sh[2] + sh[3]);
      const float v = h[(long)b * Cr + j] > 0.f ? dh : 0.f;
      a1[(long)b * Cr + j] = v;
      sum_b += v;
    }
  }
  if (t == 0) db1[j] = accumulate ? db1[j] + sum_b : sum_b;
}

// one thread per channel c: dW1[j][c] (+)= sum_b a1[b][j] mean[b][c]; g[b][c] = (sum_j W1[j][c] a1[b][j]) / HW
__global__ __launch_bounds__(NT) void se_gate_bwd0_kernel(const float* __restrict__ a1, const float* __restrict__ w1,
                                                          const float* __restrict__ mean, int B, int C, int Cr, float hw,
                                                          float* __restrict__ g, float* __restrict__ dw1, int accumulate) {
  const int c = blockIdx.x * NT + threadIdx.x;
  if (c >= C) return;
  for (int j = 0; j < Cr; ++j) {
    float acc = 0.f;
    for (int b = 0; b < B; ++b) acc += a1[(long)b * Cr + j] * mean[(long)b * C + c];
    float* d = dw1 + (long)j * C + c;
    *d = accumulate ? *d + acc : acc;
  }
  for (int b = 0; b < B; ++b) {
    float acc = 0.f;
    for (int j = 0; j < Cr; ++j) acc += w1[(long)j * C + c] * a1[(long)b * Cr + j];
    g[(long)b * C + c] = acc / hw;
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
bool bad_act(const void* p, int ld, int C) { return !p || ld < C || ld % 8 || !aligned16(p); }
int check_dims(int B, long HW, int C) {
  if (B < 1 || B > 65535 || HW < 1 || C < 8 || C % 8 || (double)B * (double)HW >= 2147483648.0) return SSA_EINVAL;
  return SSA_OK;
}
int check_gate(int B, long HW, int C, int Cr) {
  if (const int rc = check_dims(B, HW, C)) return rc;
  if (Cr < 1) return SSA_EINVAL;
  return Cr > kMaxCr || Cr > C ? SSA_EUNSUPPORTED : SSA_OK;
}
int grid_for(long n) { return (int)((n + NT - 1) / NT > 16384 ? 16384 : (n + NT - 1) / NT); }

size_t ws_floats(int B, long HW, int C, int Cr) {
  const size_t red = (size_t)B * plan_reduce(B, HW, C).nsplit * C, gate = (size_t)B * ((size_t)C + Cr);
  return red > gate ? red : gate;
}

}  // namespace

extern "C" {

int ssa_se_plan(int B, long HW, int C, int Cr, size_t* ws_bytes) {
  if (const int rc = check_gate(B, HW, C, Cr)) return rc;
  if (!ws_bytes) return SSA_EINVAL;
  *ws_bytes = ws_floats(B, HW, C, Cr) * sizeof(float);
  return SSA_OK;
}

int ssa_se_squeeze_gate(const void* y, int ldy, int B, long HW, int C, int Cr, const float* w1, const float* b1,
                        const float* w2, const float* b2, float* mean, float* h, float* s, void* ws, void* stream) {
  if (const int rc = check_gate(B, HW, C, Cr)) return rc;
  if (bad_act(y, ldy, C) || !w1 || !b1 || !w2 || !b2 || !mean || !h || !s || !ws) return SSA_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const Plan p = plan_reduce(B, HW, C);
  hipLaunchKernelGGL(se_partial_kernel<0>, dim3(p.nsplit, p.tiles, B), dim3(NT), 0, st, (const bf16_t*)y, ldy,
                     (const bf16_t*)nullptr, 0, (const bf16_t*)nullptr, 0, HW, C, 0, (float*)ws);
  SSA_LAUNCH_CHECK();
  hipLaunchKernelGGL(se_finish_kernel, dim3((C + 31) / 32, B), dim3(NT), 0, st, (const float*)ws, p.nsplit, C, (float)HW, mean);
  SSA_LAUNCH_CHECK();
  hipLaunchKernelGGL(se_fc_kernel<0>, dim3((Cr + 3) / 4, B), dim3(NT), 0, st, w1, b1, (const float*)mean, C, Cr, h);
  SSA_LAUNCH_CHECK();
  hipLaunchKernelGGL(se_fc_kernel<1>, dim3((C + 3) / 4, B), dim3(NT), 0, st, w2, b2, (const float*)h, Cr, C, s);
  SSA_LAUNCH_CHECK();
  return SSA_OK;
}

int ssa_se_apply(const void* y, int ldy, const void* r, int ldr, const float* s, void* z, int ldz, int B, long HW, int C,
                 int relu, void* stream) {
  if (const int rc = check_dims(B, HW, C)) return rc;
  if (bad_act(y, ldy, C) || bad_act(z, ldz, C) || !s || (r && bad_act(r, ldr, C))) return SSA_EINVAL;
  const long n = (long)B * HW * (C >> 3);
  if (r)
    hipLaunchKernelGGL(se_apply_kernel<true>, dim3(grid_for(n)), dim3(NT), 0, (hipStream_t)stream, (const bf16_t*)y, ldy,
                       (const bf16_t*)r, ldr, s, (bf16_t*)z, ldz, n, HW, C, relu ? 1 : 0);
  else
    hipLaunchKernelGGL(se_apply_kernel<false>, dim3(grid_for(n)), dim3(NT), 0, (hipStream_t)stream, (const bf16_t*)y, ldy,
                       (const bf16_t*)nullptr, 0, s, (bf16_t*)z, ldz, n, HW, C, relu ? 1 : 0);
  SSA_LAUNCH_CHECK();
  return SSA_OK;
}

int ssa_se_bwd_reduce(const void* dz, int lddz, const void* z, int ldz, const void* y, int ldy, int B, long HW, int C,
                      int relu, float* ds, void* ws, void* stream) {
  if (const int rc = check_dims(B, HW, C)) return rc;
  if (bad_act(dz, lddz, C) || bad_act(y, ldy, C) || (relu && bad_act(z, ldz, C)) || !ds || !ws) return SSA_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const Plan p = plan_reduce(B, HW, C);
  hipLaunchKernelGGL(se_partial_kernel<1>, dim3(p.nsplit, p.tiles, B), dim3(NT), 0, st, (const bf16_t*)y, ldy,
                     (const bf16_t*)dz, lddz, (const bf16_t*)z, ldz, HW, C, relu ? 1 : 0, (float*)ws);
  SSA_LAUNCH_CHECK();
  hipLaunchKernelGGL(se_finish_kernel, dim3((C + 31) / 32, B), dim3(NT), 0, st, (const float*)ws, p.nsplit, C, 1.f, ds);
  SSA_LAUNCH_CHECK();
  return SSA_OK;
}

int ssa_se_gate_bwd(const float* ds, const float* s, const float* h, const float* mean, const float* w1, const float* w2,
                    int B, long HW, int C, int Cr, float* g, float* dw1, float* db1, float* dw2, float* db2, int accumulate,
                    void* ws, void* stream) {
  if (const int rc = check_gate(B, HW, C, Cr)) return rc;
  if (!ds || !s || !h || !mean || !w1 || !w2 || !g || !dw1 || !db1 || !dw2 || !db2 || !ws) return SSA_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  float* a2 = (float*)ws;
  float* a1 = a2 + (size_t)B * C;
  const int acc = accumulate ? 1 : 0;
  hipLaunchKernelGGL(se_gate_bwd2_kernel, dim3((C + 3) / 4), dim3(NT), 0, st, ds, s, h, B, C, Cr, a2, dw2, db2, acc);
  SSA_LAUNCH_CHECK();
  hipLaunchKernelGGL(se_gate_bwd1_kernel, dim3(Cr), dim3(NT), 0, st, (const float*)a2, w2, h, B, C, Cr, a1, db1, acc);
  SSA_LAUNCH_CHECK();
  hipLaunchKernelGGL(se_gate_bwd0_kernel, dim3((C + NT - 1) / NT), dim3(NT), 0, st, (const float*)a1, w1, mean, B, C, Cr,
                     (float)HW, g, dw1, acc);
  SSA_LAUNCH_CHECK();
  return SSA_OK;
}

int ssa_se_apply_bwd(const void* dz, int lddz, const void* z, int ldz, const float* s, const float* g, int B, long HW, int C,
                     int relu, void* dy, int lddy, void* dr, int lddr, void* stream) {
  if (const int rc = check_dims(B, HW, C)) return rc;
  if (bad_act(dz, lddz, C) || bad_act(dy, lddy, C) || (relu && bad_act(z, ldz, C)) || !s || !g || (dr && bad_act(dr, lddr, C)))
    return SSA_EINVAL;
  const long n = (long)B * HW * (C >> 3);
  if (dr)
    hipLaunchKernelGGL(se_apply_bwd_kernel<true>, dim3(grid_for(n)), dim3(NT), 0, (hipStream_t)stream, (const bf16_t*)dz, lddz,
                       (const bf16_t*)z, ldz, s, g, (bf16_t*)dy, lddy, (bf16_t*)dr, lddr, n, HW, C, relu ? 1 : 0);
  else
    hipLaunchKernelGGL(se_apply_bwd_kernel<false>, dim3(grid_for(n)), dim3(NT), 0, (hipStream_t)stream, (const bf16_t*)dz, lddz,
                       (const bf16_t*)z, ldz, s, g, (bf16_t*)dy, lddy, (bf16_t*)nullptr, 0, n, HW, C, relu ? 1 : 0);
  SSA_LAUNCH_CHECK();
  return SSA_OK;
}

}  // extern "C"
