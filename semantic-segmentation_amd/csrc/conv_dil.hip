// 3x3 stride-1 "same" convolution with a DIFFERENT dilation on each axis, NHWC 16-bit activations, fp32 accumulate on
// MFMA (gfx950): forward, data gradient and weight gradient of
//   nn.Conv2d(Cin, Cout, 3, stride = 1, padding = (dh, dw), dilation = (dh, dw), bias = False)    network/utils.py:249-260
// the five convs of the Dense Prediction Cell (DPC; rates (1,6) (18,15) (6,21) (1,1) (6,3), doubled at output stride 8).
//
// A halo tile is the wrong shape here (the halo of (36,30) is 73 x 61 pixels around one row), so the conv is nine
// SHIFTED 1x1 GEMMs that accumulate in the same registers:
//   * a workgroup owns 64 consecutive pixels of ONE image (flat index oy * W + ox, so a tile never holds rows of two
//     images) x 256 output channels; its four waves own four 64-channel slices, a wave 64 pixels x 64 channels =
//     2 x 2 MFMA 32x32x16 tiles;
//   * tap (kh, kw) reads the pixel window shifted by ((kh - 1) dh, (kw - 1) dw): the A fragment of a lane is 16 bytes of
//     its shifted pixel straight from global memory, zero where iy or ix leaves [0, H) x [0, W) -- validity is per
//     pixel, a row of the next image is never read;
//   * the filter never touches LDS: MFMA-fragment order [n-block][k-step][lane][8] (ssa_pack_filter mode 2 / 3), one
//     16-byte load per lane and k-step straight into the registers the MFMA reads (conv_halo_reg.hip's scheme);
//   * a tap that is outside the image for the workgroup's WHOLE tile is dropped from the tile's tap list before the loop
//     (scalar interval arithmetic on the tile's pixel range): no loads, no MFMAs;
//   * (tap, 64-channel chunk) steps run through a register double buffer: the loads of step s + 1 are issued before
//     the 16 MFMAs of step s;
//   * epilogue: conv_epilogue.h -- rounding, BatchNorm partial sums of the rounded values (a wave holds all 64 pixels of
//     its channels: the sums leave from registers), the tile staged in LDS for 16-byte row stores.
// With stride 1 and padding = dilation on both axes the data gradient is the same conv with the flipped, transposed
// filter (ssa_pack_filter mode 3): one kernel serves both.  x and y may be disjoint channel slices of one allocation.
//
// Weight gradient: dW[co][ci][tap] = sum over pixels of dy[p][co] x[p + shift(tap)][ci].  A workgroup owns one tap and a
// 128 (co) x 128 (ci) block of it, a wave 64 x 64; stages of 64 pixels of one image are staged pixel-major in LDS (the x
// window shifted, invalid pixels zero) and the k = pixel fragments gathered from it element by element.  Workgroups
// split the stage list; their fp32 partials go to `ws` [split][tap][co][ci] and a second launch adds them in split
// order and writes (or adds to) dW in the parameter's OIHW layout: no floating-point atomics, a fixed order of sums.
// Stages (and whole taps) for which the tap is outside the image are skipped.
#include "conv_epilogue.h"
#include "group.h"
#include "../../include/semseg_hip.h"

namespace {

// Is there a pixel with flat index in [p0, p1] of a W-wide image whose row lies in [r0, r1] and column in [c0, c1]?
__device__ __forceinline__ bool any_pixel(int p0, int p1, int W, int r0, int r1, int c0, int c1) {
  if (r0 > r1 || c0 > c1) return false;
  int first = max(p0, r0 * W + c0);                    // the smallest such index >= p0
  const int r = first / W, c = first - r * W;
  if (c > c1) first = (r + 1) * W + c0;
  else if (c < c0) first = r * W + c0;
  return first <= min(p1, r1 * W + c1);
}

// Tap (kh, kw) reaches inside the image for some output pixel of [p0, p1]
__device__ __forceinline__ bool tap_live(int tap, int p0, int p1, int H, int W, int dh, int dw) {
  const int kh = tap / 3, kw = tap - kh * 3;
  const int sy = (kh - 1) * dh, sx = (kw - 1) * dw;
  return any_pixel(p0, p1, W, max(0, -sy), min(H - 1, H - 1 - sy), max(0, -sx), min(W - 1, W - 1 - sx));
}

struct DilArgs {
  const bf16_t* x; const uint4* wfrag; bf16_t* y; double* stats;
  int ldx, Cin, ldy, H, W, Cout, dil_h, dil_w, tiles;      // tiles: 64-pixel tiles per image
};

struct DilConv3 {
  typedef DilArgs Args;
  static constexpr int NT = 256;
  static constexpr int WPE = 2;                           // two workgroups per CU: 256 registers per wave
  static constexpr int BM = 64, BN = 256, CK = 64, CST = CK / 16;
  static constexpr int LDC = BN + 8;
  static constexpr size_t LDS_BYTES = (size_t)BM * LDC * 2;

  static __device__ __forceinline__ void run(const Args& a, const int bx, const int by, const int /*gx*/) {
    SSA_DYN_LDS(unsigned char, smem);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wn = __builtin_amdgcn_readfirstlane(tid >> 6);    // the wave's 64-channel slice
    const int H = a.H, W = a.W, HW = H * W, ldx = a.ldx, Cout = a.Cout;
    const int dh = a.dil_h, dw = a.dil_w;
    const int b = bx / a.tiles, t = bx - b * a.tiles;
    const int p0 = t * BM, p1 = min(p0 + BM, HW) - 1;
    const int n0 = by * BN;
    const bool wave_live = n0 + wn * 64 < Cout;                   // (Cout % 64 == 0: a slice is whole or absent)
    const int csteps = a.Cin / 16, nchunk = a.Cin / CK;

    f32x16_t acc[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

    if (wave_live) {
      // the tile's tap list, 4 bits per entry
      unsigned long long taps = 0;
      int ntap = 0;
      for (int tap = 0; tap < 9; ++tap)
        if (tap_live(tap, p0, p1, H, W, dh, dw)) { taps |= (unsigned long long)tap << (4 * ntap); ++ntap; }
      const int steps = ntap * nchunk;

      // A: this lane's two pixels (rows lane & 31 of the two 32-pixel blocks), k half lane >> 5
      int oy[2], ox[2];
      bool live[2];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) {
        const int p = p0 + mi * 32 + (lane & 31);
        live[mi] = p <= p1;
        const int pc = live[mi] ? p : p1;
        oy[mi] = pc / W;
        ox[mi] = pc - oy[mi] * W;
      }
      const bf16_t* xb = a.x + (long)b * HW * ldx + ((lane >> 5) << 3);
      // B: the wave's two n-blocks, one 1 KiB fragment block per (n-block, k-step)
      const int ksteps = 9 * csteps;
      const unsigned char* wq[2];
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
        wq[ni] = reinterpret_cast<const unsigned char*>(a.wfrag + (long)((n0 >> 5) + wn * 2 + ni) * ksteps * 64) + lane * 16;

      int l_ti = 0, l_chunk = 0;                                  // the step the next load() fetches
      auto load = [&](bf16x8_t (&A)[2][CST], bf16x8_t (&Bq)[2][CST]) {
        const int tap = (int)((taps >> (4 * l_ti)) & 15);
        const int kh = tap / 3, kw = tap - kh * 3;
        const int sy = (kh - 1) * dh, sx = (kw - 1) * dw;
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) {
          const int iy = oy[mi] + sy, ix = ox[mi] + sx;
          const bool ok = live[mi] && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
          const bf16_t* src = xb + ((long)iy * W + ix) * ldx + l_chunk * CK;
#pragma unroll
          for (int j = 0; j < CST; ++j) {
            uint4 raw = make_uint4(0, 0, 0, 0);
            if (ok) raw = *reinterpret_cast<const uint4*>(src + j * 16);
            A[mi][j] = __builtin_bit_cast(bf16x8_t, raw);
          }
        }
        const long k0 = (long)(tap * csteps + l_chunk * CST) * 1024;
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
          for (int j = 0; j < CST; ++j) Bq[ni][j] = *reinterpret_cast<const bf16x8_t*>(wq[ni] + k0 + j * 1024);
        if (++l_chunk == nchunk) { l_chunk = 0; ++l_ti; }
      };
      auto mma = [&](const bf16x8_t (&A)[2][CST], const bf16x8_t (&Bq)[2][CST]) {
#pragma unroll
        for (int j = 0; j < CST; ++j)
#pragma unroll
          for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = ssa_mfma32(A[mi][j], Bq[ni][j], acc[mi][ni]);
      };

      bf16x8_t A0[2][CST], B0[2][CST], A1[2][CST], B1[2][CST];
      if (steps > 0) load(A0, B0);
      for (int s = 0; s < steps; s += 2) {
        if (s + 1 < steps) load(A1, B1);
        mma(A0, B0);
        if (s + 1 < steps) {
          if (s + 2 < steps) load(A0, B0);
          mma(A1, B1);
        }
      }
    }

    // ---- epilogue: rounding to 16 bits, BatchNorm partial sums of the ROUNDED values, the tile through LDS
    double* __restrict__ stats = a.stats;
    bf16_t* Cs = reinterpret_cast<bf16_t*>(smem);
    if (wave_live) {
      double* st = stats ? stats + (long)(bx % ssa::kStatReplicas) * 2 * Cout : nullptr;
      ssa::epi_stage<LDC>(acc, nullptr, stats != nullptr, 0, wn * 64, n0, Cout, Cs, lane,
                          [&](int row) { return p0 + row <= p1; },
                          [&](int, int n, float sv, float qv) {
                            if (n < Cout) {
                              atomicAdd(&st[n], (double)sv);
                              atomicAdd(&st[Cout + n], (double)qv);
                            }
                          });
    }
    __syncthreads();
    bf16_t* yb = a.y + ((long)b * HW + p0) * a.ldy;
    const int ldy = a.ldy;
    ssa::epi_store_rows<BM, BN, NT>(Cs, n0, Cout, tid, [&](int row, bf16_t*& p) {
      p = yb + (long)row * ldy;
      return p0 + row <= p1;
    });
  }
};

// ------------------------------------------------------------------------------------------------ weight gradient
struct DilWgArgs {
  const bf16_t* x; const bf16_t* dy; float* ws;
  int ldx, lddy, B, H, W, Cin, Cout, dil_h, dil_w, nsplit, stages_img, ci_tiles;
};

struct DilWgrad {
  typedef DilWgArgs Args;
  static constexpr int NT = 256;
  static constexpr int WPE = 2;
  static constexpr int BP = 64;                           // pixels per stage (4 k-steps)
  static constexpr int BC = 128, LDT = BC + 8;            // channels per operand tile, LDS row pitch (elements)
  static constexpr int IT = BP * (BC / 8) / NT;           // 16-byte pieces per thread, operand and stage
  static constexpr size_t LDS_BYTES = 2 * (size_t)BP * LDT * 2;

  static __device__ __forceinline__ void run(const Args& a, const int bx, const int by, const int /*gx*/) {
    SSA_DYN_LDS(unsigned char, smem);
    bf16_t* Ds = reinterpret_cast<bf16_t*>(smem);           // dy tile [BP][LDT]
    bf16_t* Xs = Ds + BP * LDT;                             // shifted x tile [BP][LDT]
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = w >> 1, wn = w & 1;
    const int H = a.H, W = a.W, HW = H * W, Cin = a.Cin, Cout = a.Cout;
    const int tap = by % 9, tile = by / 9;
    const int ci0 = (tile % a.ci_tiles) * BC, co0 = (tile / a.ci_tiles) * BC;
    const int kh = tap / 3, kw = tap - kh * 3;
    const int sy = (kh - 1) * a.dil_h, sx = (kw - 1) * a.dil_w;
    const bool wave_live = co0 + wm * 64 < Cout && ci0 + wn * 64 < Cin;

    f32x16_t acc[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

    // this split's stages: stage g = (image g / stages_img, pixels (g % stages_img) * BP ...)
    const int total = a.B * a.stages_img, per = (total + a.nsplit - 1) / a.nsplit;
    const int g0 = bx * per, g1 = min(g0 + per, total);
    for (int g = g0; g < g1; ++g) {
      const int b = g / a.stages_img, s = g - b * a.stages_img;
      const int p0 = s * BP, p1 = min(p0 + BP, HW) - 1;
      if (!tap_live(tap, p0, p1, H, W, a.dil_h, a.dil_w)) continue;          // (workgroup-uniform)
      __syncthreads();                                                      // the previous stage's reads are done
#pragma unroll
      for (int i = 0; i < IT; ++i) {
        const int id = tid + i * NT, row = id >> 4, pc = (id & 15) * 8;
        const int p = p0 + row;
        uint4 dv = make_uint4(0, 0, 0, 0), xv = make_uint4(0, 0, 0, 0);
        if (p <= p1) {
          if (co0 + pc < Cout) dv = *reinterpret_cast<const uint4*>(a.dy + ((long)b * HW + p) * a.lddy + co0 + pc);
          const int oy = p / W, ox = p - oy * W;
          const int iy = oy + sy, ix = ox + sx;
          if (ci0 + pc < Cin && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W)
            xv = *reinterpret_cast<const uint4*>(a.x + (((long)b * H + iy) * W + ix) * a.ldx + ci0 + pc);
        }
        *reinterpret_cast<uint4*>(Ds + row * LDT + pc) = dv;
        *reinterpret_cast<uint4*>(Xs + row * LDT + pc) = xv;
      }
      __syncthreads();
      if (wave_live) {
        // fragments: row / column = channel lane & 31 of the block, k = pixel 8 * (lane >> 5) + j of the k-step
        const bf16_t* dp = Ds + ((lane >> 5) << 3) * LDT + wm * 64 + (lane & 31);
        const bf16_t* xp = Xs + ((lane >> 5) << 3) * LDT + wn * 64 + (lane & 31);
#pragma unroll
        for (int ks = 0; ks < BP / 16; ++ks) {
          bf16x8_t af[2], bq[2];
#pragma unroll
          for (int m = 0; m < 2; ++m) {
            uint32_t qa[4], qb[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int r0 = (ks * 16 + 2 * j) * LDT + m * 32, r1 = r0 + LDT;
              qa[j] = (uint32_t)dp[r0] | ((uint32_t)dp[r1] << 16);
              qb[j] = (uint32_t)xp[r0] | ((uint32_t)xp[r1] << 16);
            }
            af[m] = __builtin_bit_cast(bf16x8_t, make_uint4(qa[0], qa[1], qa[2], qa[3]));
            bq[m] = __builtin_bit_cast(bf16x8_t, make_uint4(qb[0], qb[1], qb[2], qb[3]));
          }
#pragma unroll
          for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = ssa_mfma32(af[mi], bq[ni], acc[mi][ni]);
        }
      }
    }
    if (!wave_live) return;
    // D: column (ci) = lane & 31, rows (co) acc_row(r, lane); every element of the block is written (zeros for a tap
    // that never reaches inside the image)
    float* dst = a.ws + ((long)bx * 9 + tap) * Cout * Cin;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int co = co0 + wm * 64 + mi * 32 + ssa::acc_row(r, lane);
          const int ci = ci0 + wn * 64 + ni * 32 + (lane & 31);
          dst[(long)co * Cin + ci] = acc[mi][ni][r];
        }
  }
};

// dw[co][ci][tap] (+)= sum over the splits' partials, in split order
__global__ __launch_bounds__(256) void dilconv_wsum_kernel(const float* __restrict__ ws, int nsplit, int Cout, int Cin,
                                                           float* __restrict__ dw, int accumulate) {
  const long e = blockIdx.x * 256L + threadIdx.x, n = (long)Cout * Cin;
  if (e >= n) return;
  for (int t = 0; t < 9; ++t) {
    const float* src = ws + (long)t * n + e;
    float s = 0.f;
    for (int k = 0; k < nsplit; ++k) s += src[(long)k * 9 * n];
    dw[e * 9 + t] = accumulate ? dw[e * 9 + t] + s : s;
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// -1: a bad descriptor; -2: a form the kernels are not built for; 0: fine
int check_desc(const ssa_dilconv_desc* d) {
  if (!d || d->B < 1 || d->H < 1 || d->W < 1 || d->Cin < 1 || d->Cout < 1) return SSA_EINVAL;
  if (d->dil_h < 1 || d->dil_w < 1) return SSA_EINVAL;
  if (d->ldx < d->Cin || d->ldy < d->Cout || d->ldx % 8 || d->ldy % 8) return SSA_EINVAL;
  if ((double)d->B * d->H * d->W >= 2147483648.0) return SSA_EINVAL;
  if (d->Cin % 64 || d->Cout % 64) return SSA_EUNSUPPORTED;
  return SSA_OK;
}

// a dilation of H (W) or more puts every off-centre tap outside, whatever its value: the kernels get the clamped one
// (their shift arithmetic stays far from the int range)
int clamp_dil(int dil, int n) { return dil < n ? dil : n; }

struct WgPlan { int ci_tiles, ntile, stages_img, nsplit; };
WgPlan plan_wgrad(const ssa_dilconv_desc& d) {
  WgPlan p;
  p.ci_tiles = (d.Cin + DilWgrad::BC - 1) / DilWgrad::BC;
  p.ntile = p.ci_tiles * ((d.Cout + DilWgrad::BC - 1) / DilWgrad::BC) * 9;
  p.stages_img = (d.H * d.W + DilWgrad::BP - 1) / DilWgrad::BP;
  const long total = (long)d.B * p.stages_img;
  long ns = 768 / p.ntile;
  if (ns > 16) ns = 16;
  if (ns > total) ns = total;
  if (ns < 1) ns = 1;
  // no empty split: with per = ceil(total / ns) stages each, the last split still starts inside the list
  const long per = (total + ns - 1) / ns;
  p.nsplit = (int)((total + per - 1) / per);
  return p;
}

}  // namespace

extern "C" {

int ssa_dilconv3x3_supported(const ssa_dilconv_desc* d) { return check_desc(d) == SSA_OK ? 1 : 0; }

int ssa_dilconv3x3(const ssa_dilconv_desc* d, const void* x, const void* w_frag, void* y, double* stats, void* stream) {
  if (const int rc = check_desc(d)) return rc;
  if (!ssa::conv_ptrs_ok(x, y, w_frag)) return SSA_EINVAL;
  DilArgs a;
  a.x = (const bf16_t*)x; a.wfrag = (const uint4*)w_frag; a.y = (bf16_t*)y; a.stats = stats;
  a.ldx = d->ldx; a.Cin = d->Cin; a.ldy = d->ldy; a.H = d->H; a.W = d->W; a.Cout = d->Cout;
  a.dil_h = clamp_dil(d->dil_h, d->H); a.dil_w = clamp_dil(d->dil_w, d->W);
  a.tiles = (int)(((long)d->H * d->W + DilConv3::BM - 1) / DilConv3::BM);
  return ssa::submit<DilConv3>(a, d->B * a.tiles, (d->Cout + DilConv3::BN - 1) / DilConv3::BN, DilConv3::LDS_BYTES,
                               (hipStream_t)stream);
}

int ssa_dilconv3x3_wgrad_plan(const ssa_dilconv_desc* d, int* nsplit, size_t* ws_bytes) {
  if (const int rc = check_desc(d)) return rc;
  if (!ws_bytes) return SSA_EINVAL;
  const WgPlan p = plan_wgrad(*d);
  if (nsplit) *nsplit = p.nsplit;
  *ws_bytes = (size_t)p.nsplit * 9 * d->Cout * d->Cin * sizeof(float);
  return SSA_OK;
}

int ssa_dilconv3x3_wgrad(const ssa_dilconv_desc* d, const void* x, const void* dy, int lddy, float* dw, int accumulate,
                         void* ws, void* stream) {
  if (const int rc = check_desc(d)) return rc;
  if (!x || !dy || !dw || !ws || lddy < d->Cout || lddy % 8 || !aligned16(x) || !aligned16(dy) || !aligned16(ws))
    return SSA_EINVAL;
  const WgPlan p = plan_wgrad(*d);
  DilWgArgs a;
  a.x = (const bf16_t*)x; a.dy = (const bf16_t*)dy; a.ws = (float*)ws;
  a.ldx = d->ldx; a.lddy = lddy; a.B = d->B; a.H = d->H; a.W = d->W; a.Cin = d->Cin; a.Cout = d->Cout;
  a.dil_h = clamp_dil(d->dil_h, d->H); a.dil_w = clamp_dil(d->dil_w, d->W);
  a.nsplit = p.nsplit; a.stages_img = p.stages_img; a.ci_tiles = p.ci_tiles;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(ssa::k_single<DilWgrad>, dim3(p.nsplit, p.ntile), dim3(DilWgrad::NT), DilWgrad::LDS_BYTES, s, a);
  SSA_LAUNCH_CHECK();
  const long n = (long)d->Cout * d->Cin;
  hipLaunchKernelGGL(dilconv_wsum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const float*)ws, p.nsplit,
                     d->Cout, d->Cin, dw, accumulate ? 1 : 0);
  SSA_LAUNCH_CHECK();
  return SSA_OK;
}

}  // extern "C"
