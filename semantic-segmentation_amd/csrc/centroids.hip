// Class-uniform sampling (--class_uniform_pct, datasets/uniform.py:84-135): per image, per tile of
// calc_tile_locations and per class the centroid of the class's pixels, on the device.  The reference reads every label
// map once per (tile, class) -- `class_id in patch`, `(patch == class_id).astype(int)`, SciPy's center_of_mass -- ;
// here one integer pass over the label bytes forms, per (image, tile, class), the pixel count and the sums of the
// tile-local x and y, and a finalize launch divides.  center_of_mass forms sum/count in fp64 of exact integers below
// 2^53 and the reference truncates with int(): integer floor division gives the same number (a quotient that is not an
// integer lies at least 1/count below the next one).  Integer accumulation: the result does not depend on the order in
// which workgroups arrive.
//
// Shape of the pass.  A workgroup owns a band of rows of one tile.  A thread's unit of work is a 16-byte chunk of a row,
// aligned in memory (so a row whose address is not a multiple of 16 -- ld = W + 5 -- has a partial chunk at either end,
// read byte by byte; every chunk inside the tile's x-range is one 16-byte load).  Label maps are long runs of one value:
// a thread keeps (raw label, count, sum x, sum y) in registers and touches LDS only when the raw label changes, so a
// chunk of one value costs three adds and a chunk column that stays in one class down the band costs one flush.  The
// id2trainid table (uniform.py:112-121; 256 bytes in LDS) is applied at the flush, once per run, not per pixel.  Each
// wave has its own [C][3] table of 64-bit sums in LDS (a class filling a 2048 tile has sum_x = 2^32 - 2^21, filling a
// 4096 tile 2^35); after the band the four tables are added and only non-empty entries go out, one 64-bit global add
// per workgroup and entry.
#include "common.h"

namespace {

constexpr int NT = 256;       // threads per workgroup
constexpr int NW = NT / 64;   // waves, one LDS table each
constexpr int MAXC = 256;

typedef unsigned long long u64;

__global__ __launch_bounds__(NT) void centroid_zero_kernel(u64* __restrict__ p, long n) {
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < n; i += (long)gridDim.x * NT) p[i] = 0;
}

struct Run {           // the labels a thread has seen since its last flush: all of one raw value
  int raw;             // -1: nothing
  unsigned n;
  u64 sx, sy;
};

__device__ __forceinline__ void run_flush(Run& r, const unsigned char* lut_s, u64* tab, int C) {
  if (r.raw >= 0 && r.n) {
    const int c = lut_s[r.raw];
    if (c < C) {
      atomicAdd(&tab[c * 3 + 0], (u64)r.n);
      atomicAdd(&tab[c * 3 + 1], r.sx);
      atomicAdd(&tab[c * 3 + 2], r.sy);
    }
  }
  r.n = 0;
  r.sx = 0;
  r.sy = 0;
}

// `len` pixels of raw label `raw` on tile row y, the first at tile column x
__device__ __forceinline__ void run_feed(Run& r, int raw, int x, int y, int len, const unsigned char* lut_s, u64* tab,
                                         int C) {
  if (raw != r.raw) {
    run_flush(r, lut_s, tab, C);
    r.raw = raw;
  }
  r.n += (unsigned)len;
  r.sx += (u64)len * (u64)x + (u64)(len * (len - 1) / 2);
  r.sy += (u64)len * (u64)y;
}

// units: (image, tile, band) triples, bands fastest.  rows: rows of a band.  cpr: chunks of a row, an upper bound
// ((tile + 30) / 16: up to 15 bytes of misalignment in front); a chunk that starts at or beyond the tile's edge is empty.
__global__ __launch_bounds__(NT) void centroid_sums_kernel(const unsigned char* __restrict__ labels, int H, int W, int ld,
                                                           int tile, int C, const unsigned char* __restrict__ lut,
                                                           int tiles_x, int tiles, int bands, int rows, int cpr,
                                                           long units, u64* __restrict__ sums) {
  __shared__ u64 tab[NW][MAXC * 3];
  __shared__ unsigned char lut_s[256];
  const int tid = threadIdx.x;
  lut_s[tid] = lut ? lut[tid] : (unsigned char)tid;
  u64* mine = tab[tid >> 6];
  for (long unit = blockIdx.x; unit < units; unit += gridDim.x) {
    const int band = (int)(unit % bands);
    const long it = unit / bands;                   // image * tiles + tile
    const int t = (int)(it % tiles), img = (int)(it / tiles);
    const int x_offs = (t % tiles_x) * tile, y_offs = (t / tiles_x) * tile;
    const int y_lo = band * rows, y_hi = y_lo + rows < tile ? y_lo + rows : tile;
    for (int k = tid; k < NW * C * 3; k += NT) tab[k / (C * 3)][k % (C * 3)] = 0;
    __syncthreads();
    Run r{-1, 0u, 0ull, 0ull};
    const int items = (y_hi - y_lo) * cpr;
    for (int i = tid; i < items; i += NT) {
      const int y = y_lo + i / cpr, k = i % cpr;
      const unsigned char* row = labels + ((long)img * H + y_offs + y) * ld + x_offs;
      const int a = (int)(reinterpret_cast<uintptr_t>(row) & 15u);
      const int xs = 16 * k - a;                    // tile column of the chunk's first byte
      if (xs >= tile) continue;
      if (xs >= 0 && xs + 16 <= tile) {
        const uint4 v = *reinterpret_cast<const uint4*>(row + xs);
        const unsigned b0 = v.x & 255u;
        if (v.x == b0 * 0x01010101u && v.y == v.x && v.z == v.x && v.w == v.x) {
          run_feed(r, (int)b0, xs, y, 16, lut_s, mine, C);
        } else {
          const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int j = 0; j < 16; ++j)
            run_feed(r, (int)((w[j >> 2] >> (8 * (j & 3))) & 255u), xs + j, y, 1, lut_s, mine, C);
        }
      } else {                                      // the row's head or tail: only the bytes inside the tile
        const int lo = xs < 0 ? 0 : xs, hi = xs + 16 < tile ? xs + 16 : tile;
        for (int x = lo; x < hi; ++x) run_feed(r, (int)row[x], x, y, 1, lut_s, mine, C);
      }
    }
    run_flush(r, lut_s, mine, C);
    __syncthreads();
    u64* out = sums + it * (long)C * 3;
    for (int k = tid; k < C * 3; k += NT) {
      u64 s = 0;
#pragma unroll
      for (int w = 0; w < NW; ++w) s += tab[w][k];
      if (s) atomicAdd(&out[k], s);
    }
    __syncthreads();                                // the tables are cleared again for the next unit
  }
}

__global__ __launch_bounds__(NT) void centroid_finalize_kernel(const u64* __restrict__ sums, int tile, int C, int tiles_x,
                                                               int tiles, long n, int* __restrict__ centroids) {
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < n; i += (long)gridDim.x * NT) {
    const int t = (int)((i / C) % tiles);
    const u64 cnt = sums[i * 3];
    int cx = -1, cy = -1;
    if (cnt) {
      cx = (int)(sums[i * 3 + 1] / cnt) + (t % tiles_x) * tile;
      cy = (int)(sums[i * 3 + 2] / cnt) + (t / tiles_x) * tile;
    }
    centroids[i * 2] = cx;
    centroids[i * 2 + 1] = cy;
  }
}

int blocks_for(long n, long cap) {
  const long b = (n + NT - 1) / NT;
  return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

}  // namespace

extern "C" {

int ssa_class_centroids_u8(const unsigned char* labels, int N, int H, int W, int ld, int tile, int C,
                           const unsigned char* lut, unsigned long long* sums, int* centroids, void* stream) {
  if (!labels || !sums || !centroids || N < 0 || H < 0 || W < 0 || ld < W || tile < 1 || C < 1 || C > MAXC)
    return SSA_EINVAL;
  const int tiles_x = W / tile, tiles_y = H / tile;
  const long tiles = (long)tiles_x * tiles_y;
  if (tiles > 0x7fffffffL) return SSA_EINVAL;
  const long entries = (long)N * tiles * C;
  if (entries == 0) return SSA_OK;                  // no image, or an image smaller than a tile: nothing to write
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(centroid_zero_kernel, dim3(blocks_for(entries * 3, 4096)), dim3(NT), 0, s, sums, entries * 3);
  SSA_LAUNCH_CHECK();
  // a band is about 16 KiB of labels: 64 chunks of work per wave, and enough workgroups for one 1024 x 2048 map (128)
  int rows = (16384 + tile - 1) / tile;
  if (rows > tile) rows = tile;
  const int bands = (tile + rows - 1) / rows;
  const int cpr = (int)(((long)tile + 30) / 16);
  const long units = (long)N * tiles * bands;
  const int grid = (int)(units < (1L << 20) ? units : (1L << 20));
  hipLaunchKernelGGL(centroid_sums_kernel, dim3(grid), dim3(NT), 0, s, labels, H, W, ld, tile, C, lut, tiles_x, (int)tiles,
                     bands, rows, cpr, units, sums);
  SSA_LAUNCH_CHECK();
  hipLaunchKernelGGL(centroid_finalize_kernel, dim3(blocks_for(entries, 4096)), dim3(NT), 0, s, sums, tile, C, tiles_x,
                     (int)tiles, entries, centroids);
  SSA_LAUNCH_CHECK();
  return SSA_OK;
}

}  // extern "C"
