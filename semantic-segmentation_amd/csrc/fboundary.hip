// Boundary F-score (eval_mask_boundary), utils/f_boundary.py:61-233 of the reference:
//   * seg2bmap            :175-233  (full-size branch)
//   * db_eval_boundary    :110-173  (the dilation with disk(r) and the four sums)
//   * eval_mask_boundary  :61-92    (the loop over classes and images)
// The reference builds two dense boolean maps per (image, class), dilates both with a disk of up to 1,257 taps and sums
// four products, over a 10-process pool.  Here every class goes through ONE pass: a class c is a boundary class of a
// pixel iff c occurs in the pixel's 2 x 2 quad (the pair on the last row / column, nothing at the corner) and not every
// member of the quad is c -- so a pixel is a boundary for at most four classes, and a map is four bytes per pixel
// (0xFF = empty).  A boundary pixel of one map is matched iff an entry of the OTHER map within dx^2 + dy^2 <= r^2
// holds its class: the tile and its halo of the other map are staged in LDS with the set of classes that occur in them,
// the tile's boundary pixels (a minority of it) are compacted, and (pixel, disk row) items are spread over the lanes,
// rows from the centre outwards, a pixel dropping out once all its classes that occur in the staged tile are found.
// All integer: counts int64 [B][C][4] = {n_fg, n_gt, fg_match, gt_match}, exact in any order.  P, R and F are taken
// from them in float64 on the host (semseg_amd/utils/f_boundary.py).
#include "common.h"
#include "../../include/semseg_hip.h"

namespace {

constexpr int NT = 256;
constexpr int TW = 64, TH = 16;     // tile of the match kernel
constexpr int MAXR = 32;            // radius of the disk
constexpr int MAXC = 254;           // classes: 0xFF is the empty byte, and a prediction byte of 0xFF stays "no class"
constexpr unsigned EMPTY = 0xffffffffu;

// class of a pixel in both maps, 0xFF = none: ignored where the GROUND TRUTH carries the ignore label (both maps,
// f_boundary.py:133-134); a label outside [0, C) that is not the ignore label belongs to no class but is not ignored
template <typename GT>
__device__ __forceinline__ void load_pair(const unsigned char* __restrict__ pred, const GT* __restrict__ gt, long i, int C,
                                          int ignore, unsigned& lp, unsigned& lg) {
  const long g = (long)gt[i];
  const unsigned p = pred[i];
  const bool ign = g == (long)ignore;
  lg = (!ign && g >= 0 && g < C) ? (unsigned)g : 0xffu;
  lp = (!ign && p < (unsigned)C) ? p : 0xffu;
}

// the boundary classes of a quad {own, e, s, se} (members outside the quad's shape passed as copies of `own`): none if
// all four are equal, else every distinct class among them, in order of appearance, the rest 0xFF
__device__ __forceinline__ unsigned quad_entry(unsigned m0, unsigned m1, unsigned m2, unsigned m3) {
  if (m0 == m1 && m0 == m2 && m0 == m3) return EMPTY;
  const unsigned m[4] = {m0, m1, m2, m3};
  unsigned e = EMPTY;
  int cnt = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned v = m[k];
    bool take = v != 0xffu;
#pragma unroll
    for (int j = 0; j < k; ++j) take = take && m[j] != v;
    if (take) {
      e = (e & ~(0xffu << (8 * cnt))) | (v << (8 * cnt));
      ++cnt;
    }
  }
  return e;
}

// Streaming pass: ent[0] = the prediction's map, ent[1] = the ground truth's, one 32-bit entry per pixel.  grid (row
// chunks of 256 pixels in strides, B).  Also clears the counters of the match kernel, which follows on the same stream
// (no memset, no host step).  Capture into a graph is NOT supported: semseg_amd/utils/f_boundary.py refuses it.
template <typename GT>
__global__ __launch_bounds__(NT) void fb_entries_kernel(const unsigned char* __restrict__ pred, const GT* __restrict__ gt,
                                                        int H, int W, int C, int ignore, unsigned* __restrict__ ent,
                                                        long plane, int64_t* __restrict__ counts, int ncounts) {
  const int b = blockIdx.y;
  if (b == 0)
    for (int i = blockIdx.x * NT + threadIdx.x; i < ncounts; i += gridDim.x * NT) counts[i] = 0;
  const long HW = (long)H * W;
  const unsigned char* pimg = pred + (long)b * HW;
  const GT* gimg = gt + (long)b * HW;
  const int xchunks = (W + NT - 1) / NT;
  const int items = H * xchunks;
  for (int it = blockIdx.x; it < items; it += gridDim.x) {
    const int y = it / xchunks;
    const int x = (it - y * xchunks) * NT + threadIdx.x;
    if (x >= W) continue;
    const long p = (long)y * W + x;
    unsigned ep = EMPTY, eg = EMPTY;
    const bool right = x + 1 < W, down = y + 1 < H;
    if (right || down) {                    // (the bottom-right pixel is never a boundary, f_boundary.py:220)
      unsigned p0, g0, p1, g1, p2, g2, p3, g3;
      load_pair(pimg, gimg, p, C, ignore, p0, g0);
      p1 = p2 = p3 = p0;
      g1 = g2 = g3 = g0;
      if (right) load_pair(pimg, gimg, p + 1, C, ignore, p1, g1);
      if (down) load_pair(pimg, gimg, p + W, C, ignore, p2, g2);
      if (right && down) load_pair(pimg, gimg, p + W + 1, C, ignore, p3, g3);
      // last row: the pair {own, e} (:218); last column: the pair {own, s} (:219)
      if (!down) { p2 = p3 = p0; g2 = g3 = g0; }
      if (!right) { p1 = p3 = p0; g1 = g3 = g0; }
      ep = quad_entry(p0, p1, p2, p3);
      eg = quad_entry(g0, g1, g2, g3);
    }
    ent[(long)b * HW + p] = ep;
    ent[plane + (long)b * HW + p] = eg;
  }
}

// Match pass.  grid (tiles in strides, B, 2): z = 0 counts the prediction's boundary pixels (n_fg) and those of them
// inside the dilated ground-truth boundary (fg_match), z = 1 the other way round (n_gt, gt_match).
__global__ __launch_bounds__(NT) void fb_match_kernel(const unsigned* __restrict__ ent, long plane, int H, int W, int C,
                                                      int r, int64_t* __restrict__ counts) {
  SSA_DYN_LDS(unsigned, stage);             // [TH + 2r][TW + 2r] entries of the other map, EMPTY outside the image
  __shared__ unsigned list_ent[TH * TW];    // the tile's boundary pixels, compacted: entry,
  __shared__ unsigned short list_pos[TH * TW];  // position in the tile,
  __shared__ unsigned found[TH * TW];       // and which of its (up to four) classes have been found so far
  __shared__ unsigned hist[MAXC * 4];
  __shared__ int halfw[MAXR + 1];           // widest dx of the disk's row |dy|
  __shared__ int npix;
  __shared__ unsigned present[8];           // bit c: class c occurs in the staged tile
  const int b = blockIdx.y, d = blockIdx.z;
  const long HW = (long)H * W;
  const unsigned* own = ent + (long)d * plane + (long)b * HW;
  const unsigned* other = ent + (long)(1 - d) * plane + (long)b * HW;
  const int SW = TW + 2 * r, SH = TH + 2 * r;
  const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
  for (int i = threadIdx.x; i < C * 4; i += NT) hist[i] = 0u;
  if ((int)threadIdx.x <= r) {
    const int dy = threadIdx.x;
    int w = 0;
    while ((w + 1) * (w + 1) + dy * dy <= r * r) ++w;
    halfw[dy] = w;
  }
  for (int t = blockIdx.x; t < tiles_x * tiles_y; t += gridDim.x) {
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    const int y0 = ty * TH, x0 = tx * TW;
    __syncthreads();                        // the previous tile's readers are done (and hist, halfw are written)
    if (threadIdx.x == 0) npix = 0;
    if (threadIdx.x < 8) present[threadIdx.x] = 0u;
    __syncthreads();
    for (int i = threadIdx.x; i < SH * SW; i += NT) {
      const int sy = i / SW, sx = i - sy * SW;
      const int y = y0 - r + sy, x = x0 - r + sx;
      const unsigned v = (y >= 0 && y < H && x >= 0 && x < W) ? other[(long)y * W + x] : EMPTY;
      stage[i] = v;
      if (v != EMPTY) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const unsigned c = (v >> (8 * q)) & 0xffu;
          if (c != 0xffu && !((present[c >> 5] >> (c & 31u)) & 1u)) atomicOr(&present[c >> 5], 1u << (c & 31u));
        }
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < TH * TW; i += NT) {
      const int ly = i / TW, lx = i - ly * TW;
      const int y = y0 + ly, x = x0 + lx;
      if (y < H && x < W) {
        const unsigned e = own[(long)y * W + x];
        if (e != EMPTY) {
          const int k = atomicAdd(&npix, 1);
          list_ent[k] = e;
          list_pos[k] = (unsigned short)i;
          found[k] = 0u;
        }
      }
    }
    __syncthreads();
    const int n = npix;
    // item w = (ring k, pixel i): k = 0 is the disk's centre row, then dy = +1, -1, +2, -2, ...
    const int total = n * (2 * r + 1);
    for (int w = threadIdx.x; w < total; w += NT) {
      const int k = w / n, i = w - k * n;
      const unsigned e = list_ent[i];
      unsigned need = 0u;           // the pixel's classes that occur anywhere in the staged tile: no other can match
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const unsigned c = (e >> (8 * q)) & 0xffu;
        if (c != 0xffu && ((present[c >> 5] >> (c & 31u)) & 1u)) need |= 1u << q;
      }
      // a plain read beside other lanes' atomicOr of the same word: bits are only ever set, so a stale value costs a
      // scan that finds the class again, never a count (the counts read found[] behind the barrier below)
      unsigned miss = need & ~found[i];
      if (miss == 0u) continue;             // every class of this pixel has been found by an earlier row
      const int dy = (k & 1) ? (k + 1) / 2 : -(k / 2);
      const int hw = halfw[dy < 0 ? -dy : dy];
      const int pos = list_pos[i];
      const int ly = pos / TW, lx = pos - ly * TW;
      const unsigned* row = stage + (ly + r + dy) * SW + lx + r;
      unsigned hit = 0u;
      for (int dx = -hw; dx <= hw && miss; ++dx) {
        const unsigned v = row[dx];
        if (v == EMPTY) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if ((miss >> q) & 1u) {
            const unsigned z = v ^ (((e >> (8 * q)) & 0xffu) * 0x01010101u);
            if ((z - 0x01010101u) & ~z & 0x80808080u) {     // some byte of the entry is this class
              miss &= ~(1u << q);
              hit |= 1u << q;
            }
          }
      }
      if (hit) atomicOr(&found[i], hit);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += NT) {
      const unsigned e = list_ent[i], f = found[i];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const unsigned c = (e >> (8 * q)) & 0xffu;
        if (c != 0xffu) {
          atomicAdd(&hist[c * 4 + d], 1u);
          if ((f >> q) & 1u) atomicAdd(&hist[c * 4 + 2 + d], 1u);
        }
      }
    }
  }
  __syncthreads();
  // the workgroup's histogram into the image's int64 counters: one atomic per non-empty bin
  unsigned long long* dst = reinterpret_cast<unsigned long long*>(counts) + (long)b * C * 4;
  for (int i = threadIdx.x; i < C * 4; i += NT)
    if (hist[i]) atomicAdd(dst + i, (unsigned long long)hist[i]);
}

inline int strided_grid(long items, int per_item, int cap) {
  long g = items, per = cap / per_item;
  if (per < 1) per = 1;
  if (g > per) g = per;
  if (g < 1) g = 1;
  return (int)g;
}

}  // namespace

extern "C" {

int ssa_fboundary_workspace_bytes(int B, int H, int W, size_t* bytes) {
  if (!bytes || B <= 0 || H <= 0 || W <= 0 || B > 65535) return SSA_EINVAL;
  *bytes = (size_t)8 * (size_t)B * (size_t)H * (size_t)W;
  return SSA_OK;
}

int ssa_fboundary_counts(const unsigned char* pred_u8, const void* gts, int gts_u8, int B, int H, int W, int C,
                         int ignore_label, int radius, int64_t* counts, void* workspace, size_t workspace_bytes,
                         void* stream) {
  if (!pred_u8 || !gts || !counts || !workspace) return SSA_EINVAL;
  if (B <= 0 || H <= 0 || W <= 0 || B > 65535) return SSA_EINVAL;
  if (C < 1 || C > MAXC) return SSA_EUNSUPPORTED;
  if (radius < 0 || radius > MAXR) return SSA_EUNSUPPORTED;
  const long tiles = (long)((W + TW - 1) / TW) * ((H + TH - 1) / TH);
  const long chunks = (long)H * ((W + NT - 1) / NT);
  if (tiles > 0x7fffffffL || chunks > 0x7fffffffL) return SSA_EUNSUPPORTED;
  const long plane = (long)B * H * W;
  if ((reinterpret_cast<uintptr_t>(workspace) & 3u) != 0 || workspace_bytes < (size_t)8 * (size_t)plane) return SSA_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  unsigned* ent = reinterpret_cast<unsigned*>(workspace);
  const dim3 g1(strided_grid(chunks, B, 16384), B);
  if (gts_u8)
    hipLaunchKernelGGL(fb_entries_kernel<unsigned char>, g1, dim3(NT), 0, s, pred_u8, (const unsigned char*)gts, H, W, C,
                       ignore_label, ent, plane, counts, B * C * 4);
  else
    hipLaunchKernelGGL(fb_entries_kernel<int64_t>, g1, dim3(NT), 0, s, pred_u8, (const int64_t*)gts, H, W, C,
                       ignore_label, ent, plane, counts, B * C * 4);
  SSA_LAUNCH_CHECK();
  // the staged tile: 40 KB at radius 32, on top of 15 KB of static LDS -- below the default 64 KB limit
  const size_t lds = (size_t)(TH + 2 * radius) * (TW + 2 * radius) * sizeof(unsigned);
  hipLaunchKernelGGL(fb_match_kernel, dim3(strided_grid(tiles, 2 * B, 16384), B, 2), dim3(NT), lds, s, ent, plane, H, W, C,
                     radius, counts);
  SSA_LAUNCH_CHECK();
  return SSA_OK;
}

}  // extern "C"
