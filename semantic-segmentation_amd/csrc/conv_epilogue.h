// The staged epilogue the MFMA forward-conv kernels share (conv_halo_gemm / conv_halo_reg / conv_gemm_wide /
// conv_tile / conv_igemm .hip; conv_tile_p.hip takes the replica count):
//   1. bias, rounding to the 16-bit storage type, the tile into LDS            epi_stage
//      with the BatchNorm partial sums of the ROUNDED values per column,
//   2. the waves' partial sums added up and sent to one stats replica          epi_reduce_stats
//      with fp64 atomics,
//   3. the staged tile stored in 16-byte rows, with a scalar channel tail      epi_store_rows
// The staged tile is [BM rows][BN + 8] elements (the 8 keep the 16 lanes of a ds_write on distinct banks), the partial
// sums behind it [wave rows][2][BN] floats; a kernel with aux inputs or an affine store keeps that ONE loop local and
// uses the rest.
#pragma once
#include "common.h"

namespace ssa {

// BatchNorm partial sums are spread over this many replicas ([replica][2][C] fp64; atomic contention); workgroup bx
// adds into replica bx % kStatReplicas.  ssa_bn_stat_replicas() hands it to whoever sizes a stats buffer.
constexpr int kStatReplicas = 8;

// Row of element r (0..15) of a lane's 32x32 MFMA accumulator (the column is lane & 31)
__device__ __forceinline__ int acc_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// A wave's MI x NI accumulator tiles, whose first row / column in the workgroup tile are row0 / col0: + bias, rounded,
// into Cs (row stride LDC).  With `stats` the sum and the sum of squares of the rounded values over the rows that
// valid(row) keeps go, per column, to sink(col, n, sum, sum of squares) on the lanes 0..31 (n = n0 + col, the channel).
template <int LDC, int MI, int NI, class Valid, class Sink>
__device__ __forceinline__ void epi_stage(const f32x16_t (&acc)[MI][NI], const float* __restrict__ bias, const bool stats,
                                          const int row0, const int col0, const int n0, const int Cout, bf16_t* Cs,
                                          const int lane, Valid valid, Sink sink) {
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) {
    const int col = col0 + ni * 32 + (lane & 31);
    const int n = n0 + col;
    const float bv = (bias != nullptr && n < Cout) ? bias[n] : 0.f;
    float sacc = 0.f, qacc = 0.f;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = row0 + mi * 32 + acc_row(r, lane);
        const bf16_t o = f2bf(acc[mi][ni][r] + bv);
        Cs[row * LDC + col] = o;
        if (stats) {
          const float f = valid(row) ? bf2f(o) : 0.f;
          sacc += f;
          qacc += f * f;
        }
      }
    if (stats) {
      sacc += __shfl_xor(sacc, 32, 64);
      qacc += __shfl_xor(qacc, 32, 64);
      if (lane < 32) sink(col, n, sacc, qacc);
    }
  }
}

// The sink that leaves a wave row's sums in LDS for epi_reduce_stats: red = [WGM][2][BN] floats
template <int BN> struct EpiRedSink {
  float* red; int wm;
  __device__ __forceinline__ void operator()(int col, int, float s, float q) const {
    red[(wm * 2 + 0) * BN + col] = s;
    red[(wm * 2 + 1) * BN + col] = q;
  }
};

// red[WGM][2][BN] -> replica bx % kStatReplicas of stats, one fp64 atomic per channel and sum, by all NT threads (a
// barrier lies between the sinks and this).  The fp32 sum over the wave rows is a tree, (0 + 1) + (2 + 3); TREE = false
// adds them left to right, conv_igemm.hip's order: the two round differently, and the sums are part of a kernel's result.
template <int WGM, int BN, int NT, bool TREE = true>
__device__ __forceinline__ void epi_reduce_stats(const float* red, double* __restrict__ stats, const int bx, const int n0,
                                                 const int Cout, const int tid) {
  static_assert(WGM == 1 || WGM == 2 || WGM == 4, "wave rows");
  double* st = stats + (long)(bx % kStatReplicas) * 2 * Cout;
  for (int i = tid; i < 2 * BN; i += NT) {
    const int which = i / BN, col = i - which * BN;
    const int n = n0 + col;
    if (n < Cout) {
      const float* p = red + which * BN + col;       // wave row w at p[w * 2 * BN]
      float v = p[0];
      if constexpr (WGM == 2) v += p[2 * BN];
      if constexpr (WGM == 4 && TREE) v = (v + p[2 * BN]) + (p[4 * BN] + p[6 * BN]);
      if constexpr (WGM == 4 && !TREE) v = ((v + p[2 * BN]) + p[4 * BN]) + p[6 * BN];
      atomicAdd(&st[which * Cout + n], (double)v);
    }
  }
}

// The staged tile Cs ([BM][BN + 8]) -> global memory in 16-byte pieces, the piece that straddles Cout element by
// element.  dst_row(row, p): false for a row outside the image, else p = where channel 0 of that row's pixel lies.
template <int BM, int BN, int NT, class DstRow>
__device__ __forceinline__ void epi_store_rows(const bf16_t* Cs, const int n0, const int Cout, const int tid, DstRow dst_row) {
  constexpr int LDC = BN + 8, CPR = BN / 8;            // 16-byte pieces per tile row
  for (int idx = tid; idx < BM * CPR; idx += NT) {
    const int row = idx / CPR, cp = idx - row * CPR;
    const int n = n0 + cp * 8;
    bf16_t* dst;
    if (!dst_row(row, dst) || n >= Cout) continue;
    dst += n;
    const bf16_t* src = Cs + row * LDC + cp * 8;
    if (n + 8 <= Cout) {
      *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src);
    } else {
      for (int j = 0; n + j < Cout; ++j) dst[j] = src[j];
    }
  }
}

// Input channels per K chunk of the halo kernels (conv_halo_gemm.hip, conv_halo_reg.hip); 0: Cin not supported
inline int pick_ck(int Cin) {
  if (Cin % 64 == 0) return 64;
  if (Cin % 48 == 0) return 48;
  return 0;
}

// x, y and the packed filter of a conv entry point: all there, all on 16-byte boundaries
inline bool conv_ptrs_ok(const void* x, const void* y, const void* w_frag) {
  if (!x || !y || !w_frag) return false;
  return ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(w_frag)) & 15u) == 0;
}

}  // namespace ssa
