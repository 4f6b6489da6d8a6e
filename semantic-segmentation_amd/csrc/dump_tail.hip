// ImageDumper on the device (utils/misc.py:204-417, driven from train.py:552-597): what the reference computes on one
// host core per dumped image -- the de-normalised input, the colourised label and prediction, their composite, the
// train-id -> label-id mapping of the submission and auto-labelling modes and the byte forms of the probability and the
// error mask -- as ONE streaming launch over the H x W pixels of one image.  Every line is a byte-valued function of one
// pixel of tensors the evaluation tail (eval_tail.hip) left on the device:
//   input_rgb[p][c] = u8((image[c][p] - inv_mean[c]) / inv_std[c] * 255.0f)       Normalize (sub_, div_) + ToPILImage
//   gt_rgb[p]       = palette[gts[p] & 255],   pred_rgb[p] = palette[pred[p]]      colorize_mask(..).convert('RGB')
//   comp_rgb[p][c]  = u8(a + alpha * (b - a)),  a = input_rgb[p][c], b = pred_rgb[p][c]             Image.blend
//   label_ids[p]    = id_table[pred[p]],  prob_u8[p] = u8(prob[p] * 255.0f),  err_u8[p] = (err[p] * 255) & 255
// u8(v) truncates toward zero, saturates outside [0, 256) and takes NaN to 0.  Every fp32 operation is rounded on its
// own (no FMA: the pragma below and the _rn intrinsics), the division is IEEE.
//
// Shape.  Every tensor is dense over the image, so the image is a flat array of n = H * W pixels and a row end means
// nothing.  A thread takes FOUR neighbouring pixels per step: one 16-byte load per fp32 plane and for the probability,
// two 16-byte loads for the four int64 labels, one dword for the four predictions and for the error mask; every RGB
// output is one 12-byte store (three dwords that hold the four pixels' bytes: a store never straddles two threads'
// pixels), every byte plane one dword.  Consecutive lanes, consecutive addresses on every access.  The palette and the
// id table share one 1 KB LDS table (r | g << 8 | b << 16 | id << 24): one LDS read per looked-up pixel.  The grid is
// what the chip keeps resident (256 CUs x 4 workgroups of 256) under a grid-stride loop; the n % 4 pixels at the end
// are taken one by one by the first workgroup.  Pointers that miss the alignment of their wide access (an odd view of
// a larger tensor) send the WHOLE launch down the pixel-by-pixel path: the same arithmetic, narrow accesses.
#include "common.h"
#include "../../include/semseg_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;
constexpr int kMaxBlocks = 256 * 4;          // 256 CUs x 4 workgroups: resident at <= 128 VGPRs

struct DumpArgs {
  const float* image;                        // [3][H][W] fp32, plane stride `plane`
  long plane;
  float inv_mean[3], inv_std[3];
  const int64_t* gts;
  const unsigned char* pred;
  const unsigned char* palette;              // 256 x 3 bytes
  const unsigned char* id_table;             // 256 bytes
  const float* prob;
  const unsigned char* err;
  float alpha;
  unsigned char *input_rgb, *gt_rgb, *pred_rgb, *comp_rgb, *label_ids, *prob_u8, *err_u8;
};

// truncation toward zero of a float to a byte; saturating, NaN -> 0 (fmaxf returns the other operand for a NaN)
__device__ __forceinline__ unsigned u8_trunc(float v) {
  return (unsigned)(int)fminf(fmaxf(v, 0.f), 255.f);
}

__device__ __forceinline__ unsigned denorm_byte(float x, float inv_mean, float inv_std) {
  return u8_trunc(__fmul_rn(__fdiv_rn(__fsub_rn(x, inv_mean), inv_std), 255.0f));
}

__device__ __forceinline__ unsigned blend_byte(unsigned a, unsigned b, float alpha) {
  const float fa = (float)(int)a;
  return u8_trunc(__fadd_rn(fa, __fmul_rn(alpha, __fsub_rn((float)(int)b, fa))));
}

// the three bytes of `in` blended towards those of `pr` (both r | g << 8 | b << 16)
__device__ __forceinline__ unsigned blend_rgb(unsigned in, unsigned pr, float alpha) {
  return blend_byte(in & 255u, pr & 255u, alpha) | (blend_byte((in >> 8) & 255u, (pr >> 8) & 255u, alpha) << 8) |
         (blend_byte((in >> 16) & 255u, (pr >> 16) & 255u, alpha) << 16);
}

struct U3 { unsigned x, y, z; };

// four pixels (r | g << 8 | b << 16 each) as the twelve bytes r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
__device__ __forceinline__ void store_rgb4(unsigned char* out, long q, const unsigned c[4]) {
  U3 v;
  v.x = (c[0] & 0xffffffu) | (c[1] << 24);
  v.y = ((c[1] >> 8) & 0xffffu) | (c[2] << 16);
  v.z = ((c[2] >> 16) & 0xffu) | (c[3] << 8);
  *reinterpret_cast<U3*>(out + q * 12) = v;
}

__device__ __forceinline__ void store_rgb1(unsigned char* out, long p, unsigned c) {
  out[p * 3] = (unsigned char)c;
  out[p * 3 + 1] = (unsigned char)(c >> 8);
  out[p * 3 + 2] = (unsigned char)(c >> 16);
}

// One pixel, narrow accesses: the tail of a launch and every pixel of an unaligned one
__device__ __forceinline__ void dump_pixel(const DumpArgs& a, const unsigned* tab, long p) {
  unsigned in = 0, pr = 0;
  if (a.input_rgb || a.comp_rgb) {
#pragma unroll
    for (int c = 0; c < 3; ++c) in |= denorm_byte(a.image[c * a.plane + p], a.inv_mean[c], a.inv_std[c]) << (8 * c);
    if (a.input_rgb) store_rgb1(a.input_rgb, p, in);
  }
  if (a.gt_rgb) store_rgb1(a.gt_rgb, p, tab[(unsigned)a.gts[p] & 255u]);
  if (a.pred_rgb || a.comp_rgb || a.label_ids) {
    pr = tab[a.pred[p]];
    if (a.pred_rgb) store_rgb1(a.pred_rgb, p, pr);
    if (a.comp_rgb) store_rgb1(a.comp_rgb, p, blend_rgb(in, pr, a.alpha));
    if (a.label_ids) a.label_ids[p] = (unsigned char)(pr >> 24);
  }
  if (a.prob_u8) a.prob_u8[p] = (unsigned char)u8_trunc(__fmul_rn(a.prob[p], 255.0f));
  if (a.err_u8) a.err_u8[p] = (unsigned char)(a.err[p] * 255u);
}

template <bool VEC>
__global__ __launch_bounds__(NT) void dump_tail_kernel(const DumpArgs a, long n) {
  __shared__ unsigned tab[256];
  {
    const int i = threadIdx.x;               // NT == 256: one entry per thread
    unsigned v = 0;
    if (a.palette) v = a.palette[i * 3] | (a.palette[i * 3 + 1] << 8) | (a.palette[i * 3 + 2] << 16);
    if (a.id_table) v |= (unsigned)a.id_table[i] << 24;
    tab[i] = v;
  }
  __syncthreads();
  const long stride = (long)gridDim.x * NT;
  const long first = blockIdx.x * (long)NT + threadIdx.x;
  if (!VEC) {
    for (long p = first; p < n; p += stride) dump_pixel(a, tab, p);
    return;
  }
  const long nq = n >> 2;
  const bool want_in = a.input_rgb || a.comp_rgb, want_pr = a.pred_rgb || a.comp_rgb || a.label_ids;
  for (long q = first; q < nq; q += stride) {
    // every load of the step first: they are in flight together
    float4 pl[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}, pb = {0.f, 0.f, 0.f, 0.f};
    uint4 g0 = {0u, 0u, 0u, 0u}, g1 = {0u, 0u, 0u, 0u};
    unsigned pd = 0, er = 0;
    if (want_in) {
#pragma unroll
      for (int c = 0; c < 3; ++c) pl[c] = reinterpret_cast<const float4*>(a.image + c * a.plane)[q];
    }
    if (a.gt_rgb) {
      g0 = reinterpret_cast<const uint4*>(a.gts)[2 * q];
      g1 = reinterpret_cast<const uint4*>(a.gts)[2 * q + 1];
    }
    if (want_pr) pd = reinterpret_cast<const unsigned*>(a.pred)[q];
    if (a.prob_u8) pb = reinterpret_cast<const float4*>(a.prob)[q];
    if (a.err_u8) er = reinterpret_cast<const unsigned*>(a.err)[q];

    unsigned in[4] = {0u, 0u, 0u, 0u}, pr[4] = {0u, 0u, 0u, 0u};
    if (want_in) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        in[0] |= denorm_byte(pl[c].x, a.inv_mean[c], a.inv_std[c]) << (8 * c);
        in[1] |= denorm_byte(pl[c].y, a.inv_mean[c], a.inv_std[c]) << (8 * c);
        in[2] |= denorm_byte(pl[c].z, a.inv_mean[c], a.inv_std[c]) << (8 * c);
        in[3] |= denorm_byte(pl[c].w, a.inv_mean[c], a.inv_std[c]) << (8 * c);
      }
      if (a.input_rgb) store_rgb4(a.input_rgb, q, in);
    }
    if (a.gt_rgb) {                          // the low byte of each little-endian int64
      const unsigned c[4] = {tab[g0.x & 255u], tab[g0.z & 255u], tab[g1.x & 255u], tab[g1.z & 255u]};
      store_rgb4(a.gt_rgb, q, c);
    }
    if (want_pr) {
#pragma unroll
      for (int k = 0; k < 4; ++k) pr[k] = tab[(pd >> (8 * k)) & 255u];
      if (a.pred_rgb) store_rgb4(a.pred_rgb, q, pr);
      if (a.comp_rgb) {
        unsigned c[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) c[k] = blend_rgb(in[k], pr[k], a.alpha);
        store_rgb4(a.comp_rgb, q, c);
      }
      if (a.label_ids)
        reinterpret_cast<unsigned*>(a.label_ids)[q] =
            (pr[0] >> 24) | ((pr[1] >> 24) << 8) | ((pr[2] >> 24) << 16) | ((pr[3] >> 24) << 24);
    }
    if (a.prob_u8)
      reinterpret_cast<unsigned*>(a.prob_u8)[q] =
          u8_trunc(__fmul_rn(pb.x, 255.0f)) | (u8_trunc(__fmul_rn(pb.y, 255.0f)) << 8) |
          (u8_trunc(__fmul_rn(pb.z, 255.0f)) << 16) | (u8_trunc(__fmul_rn(pb.w, 255.0f)) << 24);
    if (a.err_u8) {                          // (e * 255) & 255 on each of the four bytes
      unsigned v = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) v |= ((((er >> (8 * k)) & 255u) * 255u) & 255u) << (8 * k);
      reinterpret_cast<unsigned*>(a.err_u8)[q] = v;
    }
  }
  if (blockIdx.x == 0 && (long)threadIdx.x < n - 4 * nq) dump_pixel(a, tab, 4 * nq + threadIdx.x);
}

template <bool VEC>
__global__ __launch_bounds__(NT) void mask_u8_kernel(const float* __restrict__ mask, long n,
                                                     unsigned char* __restrict__ out) {
  const long stride = (long)gridDim.x * NT;
  const long first = blockIdx.x * (long)NT + threadIdx.x;
  if (!VEC) {
    for (long i = first; i < n; i += stride) out[i] = (unsigned char)u8_trunc(__fmul_rn(mask[i], 255.0f));
    return;
  }
  const long nq = n >> 2;
  for (long q = first; q < nq; q += stride) {
    const float4 v = reinterpret_cast<const float4*>(mask)[q];
    reinterpret_cast<unsigned*>(out)[q] = u8_trunc(__fmul_rn(v.x, 255.0f)) | (u8_trunc(__fmul_rn(v.y, 255.0f)) << 8) |
                                          (u8_trunc(__fmul_rn(v.z, 255.0f)) << 16) |
                                          (u8_trunc(__fmul_rn(v.w, 255.0f)) << 24);
  }
  const long i = 4 * nq + threadIdx.x;
  if (blockIdx.x == 0 && i < n) out[i] = (unsigned char)u8_trunc(__fmul_rn(mask[i], 255.0f));
}

inline bool aligned(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) == 0; }

// workgroups of 256 for `units` thread-steps under the grid-stride loop
inline int dump_blocks(long units) {
  const long b = (units + NT - 1) / NT;
  return (int)(b < 1 ? 1 : b < kMaxBlocks ? b : kMaxBlocks);
}

}  // namespace

extern "C" int ssa_dump_tail(const float* image, long plane_stride, const float* inv_mean3, const float* inv_std3,
                             const int64_t* gts, const unsigned char* pred, const unsigned char* palette,
                             const unsigned char* id_table, const float* prob, const unsigned char* err, float alpha,
                             int H, int W, unsigned char* input_rgb, unsigned char* gt_rgb, unsigned char* pred_rgb,
                             unsigned char* comp_rgb, unsigned char* label_ids, unsigned char* prob_u8,
                             unsigned char* err_u8, void* stream) {
  if (H < 1 || W < 1) return SSA_EINVAL;
  if (!input_rgb && !gt_rgb && !pred_rgb && !comp_rgb && !label_ids && !prob_u8 && !err_u8) return SSA_EINVAL;
  const long n = (long)H * W;
  const bool have_image = image && inv_mean3 && inv_std3 && plane_stride >= n;
  if ((input_rgb || comp_rgb) && !have_image) return SSA_EINVAL;
  if (gt_rgb && !(gts && palette)) return SSA_EINVAL;
  if ((pred_rgb || comp_rgb) && !(pred && palette)) return SSA_EINVAL;
  if (comp_rgb && !(alpha >= 0.f && alpha <= 1.f)) return SSA_EINVAL;
  if (label_ids && !(pred && id_table)) return SSA_EINVAL;
  if (prob_u8 && !prob) return SSA_EINVAL;
  if (err_u8 && !err) return SSA_EINVAL;
  DumpArgs a;
  const bool want_in = input_rgb || comp_rgb;
  a.image = want_in ? image : nullptr;
  a.plane = plane_stride;
  for (int c = 0; c < 3; ++c) {
    a.inv_mean[c] = want_in ? inv_mean3[c] : 0.f;
    a.inv_std[c] = want_in ? inv_std3[c] : 1.f;
  }
  a.gts = gt_rgb ? gts : nullptr;
  a.pred = (pred_rgb || comp_rgb || label_ids) ? pred : nullptr;
  a.palette = (gt_rgb || pred_rgb || comp_rgb) ? palette : nullptr;
  a.id_table = label_ids ? id_table : nullptr;
  a.prob = prob_u8 ? prob : nullptr;
  a.err = err_u8 ? err : nullptr;
  a.alpha = alpha;
  a.input_rgb = input_rgb; a.gt_rgb = gt_rgb; a.pred_rgb = pred_rgb; a.comp_rgb = comp_rgb;
  a.label_ids = label_ids; a.prob_u8 = prob_u8; a.err_u8 = err_u8;
  // the wide path: every pointer in use on the grid of its access (planes and labels 16 bytes, the rest 4)
  bool vec = n >= 4;
  if (a.image) vec = vec && aligned(a.image, 16) && plane_stride % 4 == 0;
  vec = vec && aligned(a.gts, 16) && aligned(a.prob, 16) && aligned(a.pred, 4) && aligned(a.err, 4);
  vec = vec && aligned(input_rgb, 4) && aligned(gt_rgb, 4) && aligned(pred_rgb, 4) && aligned(comp_rgb, 4);
  vec = vec && aligned(label_ids, 4) && aligned(prob_u8, 4) && aligned(err_u8, 4);
  if (vec) {
    hipLaunchKernelGGL(dump_tail_kernel<true>, dim3(dump_blocks(n >> 2)), dim3(NT), 0, (hipStream_t)stream, a, n);
  } else {
    hipLaunchKernelGGL(dump_tail_kernel<false>, dim3(dump_blocks(n)), dim3(NT), 0, (hipStream_t)stream, a, n);
  }
  SSA_LAUNCH_CHECK();
  return SSA_OK;
}

extern "C" int ssa_mask_u8(const float* mask, long n, unsigned char* out, void* stream) {
  if (!mask || !out || n < 1) return SSA_EINVAL;
  if (n >= 4 && aligned(mask, 16) && aligned(out, 4)) {
    hipLaunchKernelGGL(mask_u8_kernel<true>, dim3(dump_blocks(n >> 2)), dim3(NT), 0, (hipStream_t)stream, mask, n, out);
  } else {
    hipLaunchKernelGGL(mask_u8_kernel<false>, dim3(dump_blocks(n)), dim3(NT), 0, (hipStream_t)stream, mask, n, out);
  }
  SSA_LAUNCH_CHECK();
  return SSA_OK;
}
