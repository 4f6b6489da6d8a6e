// Halo-chunk implicit GEMM for the large 1x1 convolutions of the OCR / attention
// heads (gfx950 / MI355X): 1024->512 / 720->720 / 512->256 and their data
// gradients (network/ocr_utils.py:68-93,142-147), and the entry
// point that routes every large-channel head conv: the 3x3 problems to
// conv_halo_reg.hip, the large 1x1 ones to conv_gemm_wide.hip.
//
// Workgroup = 8 wave64s, output tile 256 pixels (8 rows x 32 columns) x 128
// output channels; each wave owns 64 pixels x 64 channels (2x2 MFMA 32x32x16
// tiles).  K runs over channel chunks of CK (48 or 64) input channels: the
// chunk's input tile is staged in LDS through registers, the filter in
// MFMA-fragment order ([n-block][k-step][lane][8], ssa_pack_filter mode 2/3)
// arrives by global_load_lds_dwordx4; both are double buffered.
#include "conv_epilogue.h"
#include "group.h"
#include "../../include/semseg_hip.h"
#include <stdlib.h>

namespace {

struct HaloArgs {
  const bf16_t* x; const uint4* wfrag; const float* bias; void* y; double* stats;
  int ldx, Cin, ldy, out_f32, B, H, W, Cout, nb_total, tiles_x, tiles_y;
};

// Epilogue: bias, bf16 rounding, BatchNorm partial sums of the ROUNDED values, the tile
// staged through LDS for 16-byte row stores (or plain fp32 stores for the logit convs).
struct HaloTile { int bx, nb0, b, y0, x0, wm, wn; };

__device__ __forceinline__ void halo_epilogue(const HaloArgs& a, const HaloTile& k, f32x16_t (&acc)[2][2], unsigned char* smem) {
  constexpr int NB = 4, TW = 32, BM = 256, BN = NB * 32;
  const float* __restrict__ bias = a.bias;
  void* __restrict__ yv = a.y;
  double* __restrict__ stats = a.stats;
  const int ldy = a.ldy, out_f32 = a.out_f32, H = a.H, W = a.W, Cout = a.Cout;
  const int bx = k.bx, nb0 = k.nb0, b = k.b, y0 = k.y0, x0 = k.x0, wm = k.wm, wn = k.wn;
  const int tid = threadIdx.x, lane = tid & 63;
  const int n_base = nb0 * 32 + wn * 64;
  if (out_f32) {
    float* y = reinterpret_cast<float*>(yv) + (long)b * H * W * ldy;
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const int n = n_base + ni * 32 + (lane & 31);
      const float bv = (bias != nullptr && n < Cout) ? bias[n] : 0.f;
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = (wm * 2 + mi) * 32 + ssa::acc_row(r, lane);
          const int oy = y0 + row / TW, ox = x0 + row % TW;
          if (oy < H && ox < W && n < Cout) y[((long)oy * W + ox) * ldy + n] = acc[mi][ni][r] + bv;
        }
    }
    return;
  }
  constexpr int LDC = BN + 8;
  bf16_t* Cs = reinterpret_cast<bf16_t*>(smem);
  float* red = reinterpret_cast<float*>(smem + (size_t)BM * LDC * 2);   // [4 wm][2][128]
  ssa::epi_stage<LDC>(acc, bias, stats != nullptr, wm * 64, wn * 64, nb0 * 32, Cout, Cs, lane,
                      [&](int row) { return y0 + row / TW < H && x0 + row % TW < W; }, ssa::EpiRedSink<BN>{red, wm});
  __syncthreads();
  if (stats != nullptr) ssa::epi_reduce_stats<4, BN, 512>(red, stats, bx, nb0 * 32, Cout, tid);
  bf16_t* yb = reinterpret_cast<bf16_t*>(yv) + (long)b * H * W * ldy;
  ssa::epi_store_rows<BM, BN, 512>(Cs, nb0 * 32, Cout, tid, [&](int row, bf16_t*& p) {
    const int oy = y0 + row / TW, ox = x0 + row % TW;
    p = yb + ((long)oy * W + ox) * ldy;
    return oy < H && ox < W;
  });
}

// 1x1 convs: a stage is a whole chunk -- 32 KiB of input tile + 16 KiB of filter per 12..16 MFMAs per wave, the
// L1 -> LDS path (64 B/clk/CU) is what bounds them, not the stage latency; they keep the register-staged, padded
// halo image and the double-buffered filter of round 2 (a DMA / swizzle pipeline with an LDS filter ring measured
// 109 -> 132 us on 720->720 @ 256x256: its zero-source padding pieces and duplicate filter blocks cost L1 cycles).
template <int CK>
struct ConvHaloGemm1 {
  static constexpr int KS = 1;
  // CK = 48: the pipeline is 80 KiB of LDS -- two workgroups per CU when the kernel stays within 128 registers
  // (it did by itself in round 2; with 142 the 720->720 conv ran 105 -> 136 us)
  static constexpr int WPE = CK == 48 ? 4 : 2;
  typedef HaloArgs Args;
  static constexpr int NT = 512;
  static __device__ __forceinline__ void run(const Args& a, const int bx, const int by, const int /*gx*/) {
  const bf16_t* __restrict__ x = a.x;
  const uint4* __restrict__ wfrag = a.wfrag;
  const int ldx = a.ldx, Cin = a.Cin, H = a.H, W = a.W;
  const int nb_total = a.nb_total, tiles_x = a.tiles_x, tiles_y = a.tiles_y;
  constexpr int NB = 4, TW = 32, TH = 8, R = KS / 2;
  constexpr int HW_ = TW + 2 * R, HH_ = TH + 2 * R;
  constexpr int PSB = CK * 2 + 16;
  constexpr int CP = CK / 8;
  constexpr int NPIECE = HH_ * HW_ * CP;
  constexpr int IT = (NPIECE + 511) / 512;
  constexpr int CST = CK / 16;                  // c-steps per chunk
  constexpr int TAPS = KS * KS;
  constexpr int HALO_BYTES = (HH_ * HW_ * PSB + 1023) / 1024 * 1024;
  constexpr int BST_BYTES = NB * CST * 1024;    // one (chunk, tap) stage of the filter
  SSA_DYN_LDS(unsigned char, smem);
  unsigned char* Hs = smem;                     // [2][HALO_BYTES]
  unsigned char* Bs = smem + 2 * HALO_BYTES;    // [2][BST_BYTES]

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;      // 4 x 2 waves
  int bid = bx;
  const int tx_i = bid % tiles_x; bid /= tiles_x;
  const int ty_i = bid % tiles_y; bid /= tiles_y;
  const int b = bid;
  const int nb0 = by * NB;
  const int x0 = tx_i * TW, y0 = ty_i * TH;
  const int nchunk = Cin / CK;
  const int csteps = Cin / 16;                  // c-steps per tap in the packed filter
  const int ksteps = TAPS * csteps;
  const int nstage = nchunk * TAPS;

  // this thread's halo pieces: global element offset (or -1) and LDS byte offset
  long g_off[IT];
  int l_off[IT];
  const bf16_t* xb = x + (long)b * H * W * ldx;
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int piece = tid + i * 512;
    const int pix = piece / CP, cp = piece - pix * CP;
    const int hy = pix / HW_, hx = pix - hy * HW_;
    const int iy = y0 - R + hy, ix = x0 - R + hx;
    const bool ok = piece < NPIECE && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
    g_off[i] = ok ? ((long)iy * W + ix) * ldx + cp * 8 : -1;
    l_off[i] = piece < NPIECE ? pix * PSB + cp * 16 : -1;
  }
  uint4 hv[IT];
  auto halo_load = [&](int chunk) {
#pragma unroll
    for (int i = 0; i < IT; ++i)
      hv[i] = g_off[i] >= 0 ? *reinterpret_cast<const uint4*>(xb + g_off[i] + chunk * CK)
                            : make_uint4(0, 0, 0, 0);
  };
  auto halo_store = [&](int buf) {
#pragma unroll
    for (int i = 0; i < IT; ++i)
      if (l_off[i] >= 0) *reinterpret_cast<uint4*>(Hs + buf * HALO_BYTES + l_off[i]) = hv[i];
  };
  // filter stage (chunk c, tap t): NB x CST fragment blocks of 1 KiB, 8 waves share them
  auto filt_stage = [&](int c, int t, int buf) {
    constexpr int NFRAG = NB * CST;
#pragma unroll
    for (int f = 0; f < (NFRAG + 7) / 8; ++f) {
      const int fi = f * 8 + wave;
      if (fi < NFRAG) {
        const int nb = fi / CST, j = fi - nb * CST;
        const int nbg = min(nb0 + nb, nb_total - 1);
        const uint4* src = wfrag + ((long)nbg * ksteps + t * csteps + c * CST + j) * 64 + lane;
        ssa_glds16(src, Bs + buf * BST_BYTES + fi * 1024);
      }
    }
  };

  int a_off[2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi) {
    const int m = (wm * 2 + mi) * 32 + (lane & 31);
    const int ty = m / TW, tx = m - ty * TW;
    a_off[mi] = (ty * HW_ + tx) * PSB + (lane >> 5) * 16;
  }
  f32x16_t acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

  halo_load(0);
  filt_stage(0, 0, 0);
  halo_store(0);
  __syncthreads();

  int c = 0, t = 0;
  for (int s = 0; s < nstage; ++s) {
    int cn = c, tn = t + 1;
    if (tn == TAPS) { tn = 0; cn = c + 1; }
    const bool more = s + 1 < nstage;
    if (more) filt_stage(cn, tn, (s + 1) & 1);
    const bool fetch_halo = (t == 0) && (c + 1 < nchunk);
    if (fetch_halo) halo_load(c + 1);
    const int kh = t / KS, kw = t - kh * KS;
    const unsigned char* Ha = Hs + (c & 1) * HALO_BYTES + (kh * HW_ + kw) * PSB;
    const unsigned char* Bc = Bs + (s & 1) * BST_BYTES + lane * 16;
#pragma unroll
    for (int j = 0; j < CST; ++j) {
      bf16x8_t af[2], bfr[2];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
        af[mi] = *reinterpret_cast<const bf16x8_t*>(Ha + a_off[mi] + j * 32);
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
        bfr[ni] = *reinterpret_cast<const bf16x8_t*>(Bc + ((wn * 2 + ni) * CST + j) * 1024);
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
          acc[mi][ni] = ssa_mfma32(af[mi], bfr[ni], acc[mi][ni]);
    }
    if (fetch_halo) halo_store((c + 1) & 1);
    __syncthreads();
    c = cn; t = tn;
  }
  HaloTile k = {bx, nb0, b, y0, x0, wm, wn};
  halo_epilogue(a, k, acc, smem);
  }
};

template <class K>
int launch_halo(const ssa_conv_desc& d, size_t pipe, const void* x, const void* wfrag, const float* bias, void* y,
                double* stats, hipStream_t s) {
  constexpr size_t stage = (size_t)256 * (128 + 8) * 2 + 4 * 2 * 128 * sizeof(float);
  const size_t lds = pipe > stage ? pipe : stage;
  HaloArgs a;
  a.x = (const bf16_t*)x; a.wfrag = (const uint4*)wfrag; a.bias = bias; a.y = y; a.stats = stats;
  a.ldx = d.ldx; a.Cin = d.Cin; a.ldy = d.ldy; a.out_f32 = d.out_f32; a.B = d.B; a.H = d.H; a.W = d.W;
  a.Cout = d.Cout; a.nb_total = (d.Cout + 31) / 32;
  a.tiles_x = (d.W + 31) / 32; a.tiles_y = (d.H + 7) / 8;
  return ssa::submit<K>(a, a.tiles_x * a.tiles_y * d.B, (a.nb_total + 3) / 4, lds, s);
}

template <int CK>
int launch_halo1(const ssa_conv_desc& d, const void* x, const void* wfrag, const float* bias, void* y, double* stats,
                 hipStream_t s) {
  constexpr size_t halo = ((size_t)8 * 32 * (CK * 2 + 16) + 1023) / 1024 * 1024;
  constexpr size_t bst = (size_t)4 * (CK / 16) * 1024;
  return launch_halo<ConvHaloGemm1<CK>>(d, 2 * halo + 2 * bst, x, wfrag, bias, y, stats, s);
}

}  // namespace

extern "C" {

int ssa_conv2d_halo_supported(const ssa_conv_desc* d) {
  if (!d) return 0;
  if (d->KH != d->KW || (d->KH != 3 && d->KH != 1)) return 0;
  if (d->stride != 1 || d->dil != 1 || d->transposed || d->pad != d->KH / 2) return 0;
  if (d->Ho != d->H || d->Wo != d->W) return 0;
  if (d->ldx % 8 || (!d->out_f32 && (d->Cout % 8 || d->ldy % 8))) return 0;
  // small problems (the 192/384-channel trunk branches at <= 64x64: 32 workgroups) stay on
  // conv_tile / the K-pipelined igemm, which spread them over more workgroups
  if (d->Cin < 192 || d->Cout < 64 || d->W < 32 || (long)d->B * d->H * d->W < 16384) return 0;
  if (d->KH == 3) return ssa_conv2d_halo_reg_supported(d);
  return ssa::pick_ck(d->Cin) != 0;
}

int ssa_conv2d_halo(const ssa_conv_desc* dp, const void* x, const void* w_frag, const float* bias,
                    void* y, double* stats, void* stream) {
  if (!dp || !x || !w_frag || !y) return SSA_EINVAL;
  if (!ssa_conv2d_halo_supported(dp)) return SSA_EUNSUPPORTED;
  if (!ssa::conv_ptrs_ok(x, y, w_frag)) return SSA_EINVAL;
  if (stats && dp->out_f32) return SSA_EINVAL;
  const ssa_conv_desc& d = *dp;
  hipStream_t s = (hipStream_t)stream;
  // the large 1x1 problems go to the 256 x 256 tile (conv_gemm_wide.hip); SSA_GEMM_WIDE=0: all stay here
  static const bool wide_on = !(getenv("SSA_GEMM_WIDE") && atoi(getenv("SSA_GEMM_WIDE")) == 0);
  if (wide_on && d.KH == 1 && ssa_conv2d_gemm_wide_supported(dp)) return ssa_conv2d_gemm_wide(dp, x, w_frag, bias, y, stats, stream);
  if (d.KH == 3) return ssa_conv2d_halo_reg(dp, x, w_frag, bias, y, stats, stream);
  if (ssa::pick_ck(d.Cin) == 64) return launch_halo1<64>(d, x, w_frag, bias, y, stats, s);
  return launch_halo1<48>(d, x, w_frag, bias, y, stats, s);
}

}  // extern "C"
