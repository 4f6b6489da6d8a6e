// The label half of the auto-labelled coarse data path (scripts/train_cityscapes_sota.yml: train_extra images whose
// labels a teacher wrote, merged with gtCoarse).  Two call sites of the reference do the same kind of work with one
// whole-image NumPy pass per label id (about 35 per image):
//   * the loader, BaseLoader.read_images + the thresholding of __getitem__ (datasets/base_loader.py:152-229): the drop
//     mask, `for k, v in id_to_trainid.items(): hit = (mask == k) [| (gtCoarse == k)]; mask[hit] = v` against the mask AS
//     REWRITTEN SO FAR, then `mask[prob / 255.0 < CUSTOM_COARSE_PROB] = IGNORE_LABEL`           (compare_current = 1)
//   * the centroid pass, class_centroids_image (datasets/uniform.py:104-121): the same loop with the hit taken against an
//     UNTOUCHED COPY of the mask, so that the last hitting step wins                             (compare_current = 0)
// In both the gtCoarse pixels of id k join the hit only for a boosted step whose own hit is non-empty IN THIS IMAGE.
//
// Once those per-image "is id k there at step k" bits are known, the output byte is a function of the pair
// (o, g) = (auto label after the drop mask, gtCoarse label) alone.  So, per image:
//   1. autolabel_clear_kernel     zeroes the image's 65,536-bit set of pairs
//   2. autolabel_pairs_kernel     one streaming pass over o and g: which pairs occur (a workgroup collects them in an
//                                 8 KiB bit set in LDS -- a thread touches it only when its pair changes, label maps are
//                                 long runs -- and ORs its non-zero words into the image's set)
//   3. autolabel_resolve_kernel   one workgroup per image walks the steps IN ORDER over the pairs that occur, thread o
//                                 owning the pairs (o, *): the current value of every pair lives in 64 KiB of LDS; a boosted
//                                 step first reduces "some pair that occurs has the compared value k" over the workgroup.
//                                 Nothing is assumed about the map (a value may equal a later key: chains are followed in
//                                 mode 1 and not in mode 0, as the reference does).  Writes table[o][g] of the pairs that
//                                 occur and nothing else: its work follows the number of pairs in the image (about a
//                                 hundred in a label map), not the 65,536 there could be
//   4. autolabel_apply_kernel     the second streaming pass: out = p < cut ? ignore : table[o][g], 16 bytes per store
// Four launches whatever the arguments; no host synchronisation, no allocation: the call can be captured, and since
// the bits and the table are computed on the device a replay follows the data.  The steps travel as kernel arguments.
//
// A thread's unit of work in the streaming passes is a 16-byte chunk of a row, aligned in memory on the array that
// decides (labels in pass 2, out in pass 4), so a row whose address is not a multiple of 16 -- ld = W + 5 -- has a
// partial chunk at either end, served byte by byte, as in centroids.hip.  The other arrays are read at the same x with
// the widest load their own address allows (16, 4 x 4 or 16 x 1 bytes).
#include "common.h"

namespace {

constexpr int NT = 256;          // threads per workgroup, all kernels; the resolve kernel's thread t owns o = t
constexpr int PAIR_WORDS = 2048; // 65,536 bits
constexpr int MAX_STEPS = 256;

struct Steps {                   // kernel argument: 768 bytes
  unsigned char key[MAX_STEPS], val[MAX_STEPS], boost[MAX_STEPS];
};

struct Window {                  // pixels outside [x0, x1) x [y0, y1) read as label 0 (the whole image: no drop mask)
  int x0, y0, x1, y1;
};

__global__ __launch_bounds__(NT) void autolabel_clear_kernel(unsigned* __restrict__ p, long n) {
  const long i = blockIdx.x * (long)NT + threadIdx.x;
  if (i < n) p[i] = 0;
}

__device__ __forceinline__ uint4 load16(const unsigned char* p) {
  const unsigned a = (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u);
  if (a == 0) return *reinterpret_cast<const uint4*>(p);
  uint4 v;
  if ((a & 3u) == 0) {
    const unsigned* q = reinterpret_cast<const unsigned*>(p);
    v.x = q[0]; v.y = q[1]; v.z = q[2]; v.w = q[3];
    return v;
  }
  unsigned w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
    w[i] = (unsigned)p[4 * i] | ((unsigned)p[4 * i + 1] << 8) | ((unsigned)p[4 * i + 2] << 16) | ((unsigned)p[4 * i + 3] << 24);
  v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
  return v;
}

// the bytes [lo, hi) of a 4-byte word as a mask, lo and hi relative to the word's first byte (any integers)
__device__ __forceinline__ unsigned byte_mask(int lo, int hi) {
  const unsigned below_hi = hi >= 4 ? 0xffffffffu : (hi <= 0 ? 0u : ((1u << (8 * hi)) - 1u));
  const unsigned below_lo = lo >= 4 ? 0xffffffffu : (lo <= 0 ? 0u : ((1u << (8 * lo)) - 1u));
  return below_hi & ~below_lo;
}

// the drop mask on the 16 labels at columns xs .. xs + 15 of row y
__device__ __forceinline__ uint4 window16(uint4 v, int xs, int y, const Window& w) {
  const int lo = w.x0 - xs, hi = w.x1 - xs;
  if (y < w.y0 || y >= w.y1 || hi <= 0 || lo >= 16) return make_uint4(0u, 0u, 0u, 0u);
  if (lo <= 0 && hi >= 16) return v;
  v.x &= byte_mask(lo, hi);
  v.y &= byte_mask(lo - 4, hi - 4);
  v.z &= byte_mask(lo - 8, hi - 8);
  v.w &= byte_mask(lo - 12, hi - 12);
  return v;
}

__device__ __forceinline__ bool inside(int x, int y, const Window& w) {
  return x >= w.x0 && x < w.x1 && y >= w.y0 && y < w.y1;
}

__device__ __forceinline__ bool one_value(const uint4& v) {
  return v.x == (v.x & 255u) * 0x01010101u && v.y == v.x && v.z == v.x && v.w == v.x;
}

__device__ __forceinline__ unsigned byte_of(const uint4& v, int j) {
  const unsigned w = (j >> 2) == 0 ? v.x : (j >> 2) == 1 ? v.y : (j >> 2) == 2 ? v.z : v.w;
  return (w >> (8 * (j & 3))) & 255u;
}

__device__ __forceinline__ void mark(unsigned* bits, int& last, unsigned o, unsigned g) {
  const int pair = (int)(o << 8 | g);
  if (pair != last) {
    atomicOr(&bits[pair >> 5], 1u << (pair & 31));
    last = pair;
  }
}

// One workgroup: `rows` rows of one image (bands fastest in blockIdx.x).  cpr: chunks of a row, an upper bound
// ((W + 30) / 16: up to 15 bytes of misalignment in front); a chunk that starts at or beyond W is empty.
__global__ __launch_bounds__(NT) void autolabel_pairs_kernel(const unsigned char* __restrict__ labels,
                                                             const unsigned char* __restrict__ coarse, int H, int W,
                                                             long ld_l, long ld_c, Window win, int bands, int rows, int cpr,
                                                             unsigned* __restrict__ pairs) {
  __shared__ unsigned bits[PAIR_WORDS];
  const int tid = threadIdx.x;
  const int band = (int)(blockIdx.x % (unsigned)bands), img = (int)(blockIdx.x / (unsigned)bands);
  for (int k = tid; k < PAIR_WORDS; k += NT) bits[k] = 0;
  __syncthreads();
  const int y_lo = band * rows, y_hi = y_lo + rows < H ? y_lo + rows : H;
  const int items = (y_hi - y_lo) * cpr;
  int last = -1;
  for (int i = tid; i < items; i += NT) {
    const int y = y_lo + i / cpr, k = i % cpr;
    const unsigned char* row = labels + ((long)img * H + y) * ld_l;
    const unsigned char* crow = coarse ? coarse + ((long)img * H + y) * ld_c : nullptr;
    const int xs = 16 * k - (int)(reinterpret_cast<uintptr_t>(row) & 15u);     // column of the chunk's first byte
    if (xs >= W) continue;
    if (xs >= 0 && xs + 16 <= W) {
      const uint4 o = window16(*reinterpret_cast<const uint4*>(row + xs), xs, y, win);
      const uint4 g = crow ? load16(crow + xs) : make_uint4(0u, 0u, 0u, 0u);
      if (one_value(o) && one_value(g)) {
        mark(bits, last, o.x & 255u, g.x & 255u);
      } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) mark(bits, last, byte_of(o, j), byte_of(g, j));
      }
    } else {                                        // the row's head or tail: only the bytes inside the image
      const int lo = xs < 0 ? 0 : xs, hi = xs + 16 < W ? xs + 16 : W;
      for (int x = lo; x < hi; ++x) mark(bits, last, inside(x, y, win) ? row[x] : 0u, crow ? crow[x] : 0u);
    }
  }
  __syncthreads();
  unsigned* mine = pairs + (long)img * PAIR_WORDS;
  for (int k = tid; k < PAIR_WORDS; k += NT) {
    const unsigned b = bits[k];
    if (b) atomicOr(&mine[k], b);
  }
}

// One workgroup per image; thread t owns the pairs (o = t, g = 0 .. 255): their bits are the image's words 8 t .. 8 t + 7.
// cur[g][o]: the value the pair has now, kept for the pairs that occur only (a wave's 64 threads touch 64 consecutive
// bytes: no bank conflict).
__global__ __launch_bounds__(NT) void autolabel_resolve_kernel(const unsigned* __restrict__ pairs, Steps st, int n_steps,
                                                               int compare_current, unsigned char* __restrict__ table) {
  __shared__ unsigned char cur[256 * 256];
  __shared__ int flag[3];
  const int t = threadIdx.x;
  const long img = blockIdx.x;
  unsigned pw[8];
  unsigned any = 0;
#pragma unroll
  for (int w = 0; w < 8; ++w) {
    pw[w] = pairs[img * PAIR_WORDS + t * 8 + w];
    any |= pw[w];
  }
#pragma unroll
  for (int w = 0; w < 8; ++w)
    for (unsigned b = pw[w]; b; b &= b - 1) cur[(w * 32 + __builtin_ctz(b)) * 256 + t] = (unsigned char)t;
  if (t < 3) flag[t] = 0;
  __syncthreads();
  int c = 0;                                        // boosted steps so far: which of the three flags this one uses
  for (int s = 0; s < n_steps; ++s) {
    const unsigned k = st.key[s], v = st.val[s];
    bool gate = false;
    if (st.boost[s]) {                              // uniform: the steps are kernel arguments
      bool found = false;
      if (compare_current) {
#pragma unroll
        for (int w = 0; w < 8; ++w)
          for (unsigned b = pw[w]; b; b &= b - 1) found |= cur[(w * 32 + __builtin_ctz(b)) * 256 + t] == k;
      } else {
        found = any && (unsigned)t == k;
      }
      // flag[c % 3] is zero: cleared before the first step, or two boosted steps ago before a barrier every thread
      // has passed since.  Nobody reads flag[(c + 1) % 3] any more: its readers of two boosted steps ago passed the
      // last barrier after reading it.
      if (t == 0) flag[(c + 1) % 3] = 0;
      if (found) flag[c % 3] = 1;
      __syncthreads();
      gate = flag[c % 3] != 0;
      ++c;
    }
    if (compare_current) {
#pragma unroll
      for (int w = 0; w < 8; ++w)
        for (unsigned b = pw[w]; b; b &= b - 1) {
          const unsigned g = (unsigned)(w * 32 + __builtin_ctz(b));
          if (cur[g * 256 + t] == k || (gate && g == k)) cur[g * 256 + t] = (unsigned char)v;
        }
    } else if ((unsigned)t == k) {
#pragma unroll
      for (int w = 0; w < 8; ++w)
        for (unsigned b = pw[w]; b; b &= b - 1) cur[(w * 32 + __builtin_ctz(b)) * 256 + t] = (unsigned char)v;
    } else if (gate) {                              // the pair (t, g = k), if it occurs
      unsigned word = 0;
#pragma unroll
      for (int w = 0; w < 8; ++w) word = (unsigned)w == (k >> 5) ? pw[w] : word;
      if ((word >> (k & 31)) & 1u) cur[k * 256 + t] = (unsigned char)v;
    }
  }
  unsigned char* row = table + img * 65536 + t * 256;
#pragma unroll
  for (int w = 0; w < 8; ++w)
    for (unsigned b = pw[w]; b; b &= b - 1) {
      const int g = w * 32 + __builtin_ctz(b);
      row[g] = cur[g * 256 + t];
    }
}

__device__ __forceinline__ unsigned lookup(const unsigned char* tab, int& last, unsigned& val, unsigned o, unsigned g) {
  const int pair = (int)(o << 8 | g);
  if (pair != last) {
    val = tab[pair];
    last = pair;
  }
  return val;
}

// One thread per 16-byte chunk of `out` (items = N * H * cpr, rows fastest after chunks).
__global__ __launch_bounds__(NT) void autolabel_apply_kernel(const unsigned char* __restrict__ labels,
                                                             const unsigned char* __restrict__ coarse,
                                                             const unsigned char* __restrict__ prob, int H, int W, long ld_l,
                                                             long ld_c, long ld_p, long ld_o, Window win, unsigned cut,
                                                             unsigned ignore, int cpr, long items,
                                                             const unsigned char* __restrict__ table,
                                                             unsigned char* __restrict__ out) {
  const long i = blockIdx.x * (long)NT + threadIdx.x;
  if (i >= items) return;
  const int k = (int)(i % cpr);
  const long r = i / cpr;                           // image * H + y
  const int y = (int)(r % H);
  const unsigned char* tab = table + (r / H) * 65536;
  const unsigned char* lrow = labels + r * ld_l;
  const unsigned char* crow = coarse ? coarse + r * ld_c : nullptr;
  const unsigned char* prow = cut ? prob + r * ld_p : nullptr;
  unsigned char* orow = out + r * ld_o;
  const int xs = 16 * k - (int)(reinterpret_cast<uintptr_t>(orow) & 15u);
  if (xs >= W) return;
  int last = -1;
  unsigned val = 0;
  if (xs >= 0 && xs + 16 <= W) {
    const uint4 o = window16(load16(lrow + xs), xs, y, win);
    const uint4 g = crow ? load16(crow + xs) : make_uint4(0u, 0u, 0u, 0u);
    uint4 res;
    if (!cut && one_value(o) && one_value(g)) {
      const unsigned b = tab[(o.x & 255u) << 8 | (g.x & 255u)] * 0x01010101u;
      res = make_uint4(b, b, b, b);
    } else {
      const uint4 p = prow ? load16(prow + xs) : make_uint4(0u, 0u, 0u, 0u);
      unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const unsigned b = lookup(tab, last, val, byte_of(o, j), byte_of(g, j));
        w[j >> 2] |= (prow && byte_of(p, j) < cut ? ignore : b) << (8 * (j & 3));
      }
      res = make_uint4(w[0], w[1], w[2], w[3]);
    }
    *reinterpret_cast<uint4*>(orow + xs) = res;
  } else {
    const int lo = xs < 0 ? 0 : xs, hi = xs + 16 < W ? xs + 16 : W;
    for (int x = lo; x < hi; ++x) {
      const unsigned b = lookup(tab, last, val, inside(x, y, win) ? lrow[x] : 0u, crow ? crow[x] : 0u);
      orow[x] = (unsigned char)(prow && prow[x] < cut ? ignore : b);
    }
  }
}

}  // namespace

extern "C" {

int ssa_autolabel_u8(const unsigned char* labels, const unsigned char* coarse, const unsigned char* prob, int N, int H,
                     int W, int ld_labels, int ld_coarse, int ld_prob, const unsigned char* steps, int n_steps,
                     int compare_current, int win_x0, int win_y0, int win_x1, int win_y1, int prob_cut, int ignore_label,
                     unsigned int* pairs, unsigned char* table, unsigned char* out, int ld_out, void* stream) {
  if (!labels || !pairs || !table || !out || N < 0 || H < 0 || W < 0 || ld_labels < W || ld_out < W || n_steps < 0 ||
      n_steps > MAX_STEPS || (n_steps && !steps) || prob_cut < 0 || prob_cut > 256 || (prob_cut && (!prob || ld_prob < W)) ||
      (coarse && ld_coarse < W) || ignore_label < 0 || ignore_label > 255 || (compare_current != 0 && compare_current != 1) ||
      (reinterpret_cast<uintptr_t>(pairs) & 3u) || N > (1 << 24))
    return SSA_EINVAL;
  Window win{0, 0, W, H};
  if (win_x1 > win_x0 && win_y1 > win_y0) {         // (an empty window: no drop mask)
    if (win_x0 < 0 || win_y0 < 0 || win_x1 > W || win_y1 > H) return SSA_EINVAL;
    win = Window{win_x0, win_y0, win_x1, win_y1};
  }
  Steps st;
  for (int s = 0; s < MAX_STEPS; ++s) {
    st.key[s] = s < n_steps ? steps[3 * s] : 0;
    st.val[s] = s < n_steps ? steps[3 * s + 1] : 0;
    st.boost[s] = s < n_steps && steps[3 * s + 2] ? 1 : 0;
    if (st.boost[s] && !coarse) return SSA_EINVAL;
  }
  if ((long)N * H * W == 0) return SSA_OK;          // no pixel: nothing to write
  // a band is about 16 KiB of labels, as in centroids.hip: 128 workgroups for one 1024 x 2048 map
  int rows = (16384 + W - 1) / W;
  if (rows > H) rows = H;
  const int bands = (H + rows - 1) / rows;
  const int cpr = (int)(((long)W + 30) / 16);
  const long items = (long)N * H * cpr;
  const long apply_blocks = (items + NT - 1) / NT;
  if ((long)N * bands > 0x7fffffffL || apply_blocks > 0x7fffffffL) return SSA_EINVAL;    // no launch caps its grid
  hipStream_t s = (hipStream_t)stream;
  const long words = (long)N * PAIR_WORDS;
  hipLaunchKernelGGL(autolabel_clear_kernel, dim3((unsigned)(words / NT)), dim3(NT), 0, s, pairs, words);
  SSA_LAUNCH_CHECK();
  hipLaunchKernelGGL(autolabel_pairs_kernel, dim3((unsigned)((long)N * bands)), dim3(NT), 0, s, labels, coarse, H, W,
                     (long)ld_labels, (long)ld_coarse, win, bands, rows, cpr, pairs);
  SSA_LAUNCH_CHECK();
  hipLaunchKernelGGL(autolabel_resolve_kernel, dim3((unsigned)N), dim3(NT), 0, s, pairs, st, n_steps, compare_current, table);
  SSA_LAUNCH_CHECK();
  hipLaunchKernelGGL(autolabel_apply_kernel, dim3((unsigned)apply_blocks), dim3(NT), 0, s, labels, coarse, prob, H, W,
                     (long)ld_labels, (long)ld_coarse, (long)ld_prob, (long)ld_out, win, (unsigned)prob_cut,
                     (unsigned)ignore_label, cpr, items, table, out);
  SSA_LAUNCH_CHECK();
  return SSA_OK;
}

}  // extern "C"
