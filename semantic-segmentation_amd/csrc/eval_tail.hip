// The tail of eval_minibatch (utils/trnval_utils.py:116-196, utils/misc.py:50-67, loss/utils.py:121-134) in one launch:
//   out  = ((0.0 + src_0 + src_1 + ...) / div_scales) / div_flips      flip x scale averaging, the reference's order
//   pred = first argmax_c out, prob = max_c softmax(out) = 1 / sum_c exp(out - max), err = valid && pred != gt,
//   hist[gt * C + pred] += 1, loss_acc += {(max + log sum exp) - out[gt], 1}, avg = out (only when asked for)
// Every source logit is read exactly once; what is written is per pixel (6 bytes) unless `avg` is wanted.
//
// Shape.  A workgroup owns one SEGMENT OF AN IMAGE ROW at a time (a row is cut into near-equal segments), so the mirror
// of the segment along W is again one contiguous span of the source: a mirrored source is that span with its pixels
// placed in descending order, the flip is never a tensor.  Per source the span is streamed as float4 on the 16-byte
// grid of the buffer (the span's first and last vector may reach into the neighbouring pixels; those elements are
// dropped) and summed into ONE [pixels][S] tile in LDS, source after source in argument order -- the summation order
// is the contract.  Same-orientation sources map an element to the same thread, so a barrier separates two sources only
// where the orientation changes (once for flips = [1, 0]).
// The stream never stops: the work of a workgroup is a flat sequence of STEPS (tile, source, chunk of 4 x 256 float4),
// and the loads of step i + 1 -- the next source, or the next tile's first source together with its labels -- are
// issued before step i is added into the tile, so they are in flight during the LDS pass and during the per-pixel pass
// of a finished tile (two register sets, A / B, taken in turn: no copy, hence no wait, between them).  A segment is
// sized so that a source fills whole chunks (19 classes: 215 pixels = one chunk; 65: 62; 128: 63 = two).
// Per-pixel pass: K = 1 / 2 / 4 neighbouring lanes share a pixel (every thread busy at any segment length), lane k
// takes the classes k, k + K, ...; the row stride S is K times an odd number, which keeps the K x 32 / K rows of a
// half-wave on distinct banks; partial argmax / sum are combined by cross-lane exchanges.  exp is the hardware's
// (v_exp_f32 on x * log2 e: 1 ulp plus |x| 2^-24 from the argument, |x| e^x <= 1 / e for x <= 0); a division by a power
// of two is the multiplication by its reciprocal (the same correctly rounded quotient).
// The C x C histogram is counted in LDS per workgroup and flushed with one global atomic per non-zero cell, the loss
// with two fp64 atomics, when the workgroup retires; the grid is what the chip keeps resident.  Tile + histogram are
// held to 40 KB where the class count allows (19 and 65 classes: four workgroups per CU; at 128 classes the 64 KB
// histogram leaves one).
#include "common.h"
#include "group.h"
#include "../../include/semseg_hip.h"

namespace {

constexpr int NT = 256;
constexpr int kMaxSrc = 8;
constexpr int kMaxClasses = 128;             // the limit of ssa_ce_fwd
constexpr size_t kLdsBudget = 40 * 1024;     // tile + histogram per workgroup: four workgroups per CU (160 KB)
constexpr int kChunkVecs = 4 * NT;           // float4 per step: four per thread

struct TailSrcs {
  const float* p[kMaxSrc];
  int flip[kMaxSrc];
  int n;
};

struct TailGeom {
  long rows;        // B * H image rows
  long total;       // floats of one source buffer reachable from its pointer: ((P - 1) * ld + C)
  int W, C, ld;
  int S;            // LDS row stride in floats: K * odd
  int K;            // lanes per pixel in the per-pixel pass (1, 2, 4); K * seglen <= NT
  int nseg, seglen; // segments per image row, pixels per segment (the last one may be shorter)
  int nchunk;       // steps per source and tile: nchunk * kChunkVecs float4 (or as many floats) cover any segment's span
  int vec;          // 1: ld == C >= 4 and every source pointer is 16-byte aligned -> float4 loads
  float rcp_scales, rcp_flips;   // 1 / divisor where it is a power of two (multiply), else 0 (divide)
};

struct TailRegs {   // what one step keeps in flight: four float4 (or sixteen floats) per thread and the tile's label
  float f[16];
  long lab;         // the thread's label of the step's tile
};

struct TileSpan {
  int n, nel;       // pixels, floats
  long p0, pm;      // first pixel of the segment / of its mirror image
};

__device__ __forceinline__ TileSpan tile_span(const TailGeom& g, long t) {
  TileSpan ts;
  const long row = t / g.nseg;
  const int x0 = (int)(t - row * g.nseg) * g.seglen;
  ts.n = min(g.seglen, g.W - x0);
  ts.nel = ts.n * g.C;
  ts.p0 = row * g.W + x0;
  ts.pm = row * g.W + (g.W - x0 - ts.n);
  return ts;
}

// the float4 of one (source, tile): first vector of the buffer's 16-byte grid that touches the span, their count, and
// the index of the first one's first float relative to the span (-3 .. 0)
struct SpanVecs { long q0; int nvec, r00; };
__device__ __forceinline__ SpanVecs span_vecs(const TailGeom& g, const TileSpan& ts, long ps) {
  SpanVecs sv;
  const long f0 = ps * g.C;
  sv.q0 = f0 >> 2;
  sv.nvec = (int)(((f0 + ts.nel + 3) >> 2) - sv.q0);
  sv.r00 = (int)(sv.q0 * 4 - f0);
  return sv;
}

// (pixel, class) of float `rel` of a span, and its advance by a constant number of floats (dj pixels + dc classes):
// one division per thread and step, none per load
struct PixCls { int js, c; };
__device__ __forceinline__ PixCls pix_cls(int rel, int C) {
  PixCls pc;
  pc.js = (rel < 0 ? 0 : rel) / C;
  pc.c = rel - pc.js * C;                                        // negative for the floats in front of the span
  return pc;
}
__device__ __forceinline__ void advance(PixCls& pc, int dj, int dc, int C) {
  pc.js += dj;
  pc.c += dc;
  if (pc.c >= C) { pc.c -= C; ++pc.js; }
  if (pc.c < 0 && pc.js > 0) { pc.c += C; --pc.js; }
}

__device__ __forceinline__ void issue_step(const TailSrcs& src, const TailGeom& g, const int64_t* __restrict__ labels,
                                           long t, int s, int k, TailRegs& r) {
  const TileSpan ts = tile_span(g, t);
  const float* __restrict__ sp = src.p[s];
  const long ps = src.flip[s] ? ts.pm : ts.p0;
  if (g.vec) {
    const SpanVecs sv = span_vecs(g, ts, ps);
    const long qfull = g.total >> 2;                             // vectors that lie wholly inside the buffer
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      int vi = (k * 4 + u) * NT + (int)threadIdx.x;
      if (vi >= sv.nvec) vi = 0;                                 // (loaded, not placed)
      // unconditional: a load under a branch is waited for where the branch joins.  The buffer's last, partial vector
      // (total % 4 floats; one thread of the whole grid meets it) is fetched again in place_step
      const long q = min(sv.q0 + vi, qfull - 1);
      const float4 v = reinterpret_cast<const float4*>(sp)[q];
      r.f[4 * u] = v.x; r.f[4 * u + 1] = v.y; r.f[4 * u + 2] = v.z; r.f[4 * u + 3] = v.w;
    }
  } else {      // ld != C, an unaligned base or fewer than four classes: sixteen coalesced dword loads
    PixCls pc = pix_cls(k * 16 * NT + (int)threadIdx.x, g.C);
    const int dj = NT / g.C, dc = NT - dj * g.C;
#pragma unroll
    for (int m = 0; m < 16; ++m) {
      const bool in = (k * 16 + m) * NT + (int)threadIdx.x < ts.nel;
      r.f[m] = sp[in ? (ps + pc.js) * g.ld + pc.c : ps * g.ld];
      advance(pc, dj, dc, g.C);
    }
  }
  if (labels) r.lab = (long)labels[ts.p0 + min((int)threadIdx.x / g.K, ts.n - 1)];   // (every step: no branch on s, k)
}

__device__ __forceinline__ float pick4(int k, float a, float b, float c, float d) {
  return k == 0 ? a : k == 1 ? b : k == 2 ? c : d;
}

// The loads of one step are added into the tile.  float4 mode: lane l handles its vector's components in the order
// (l / 8 + kk) % 4 -- in component order the 32 lanes of a half-wave would hit every fourth bank only (a 4-way
// conflict on each of the four accesses); a vector crosses at most one pixel boundary (C >= 4), where the LDS address
// jumps by the row padding (or, mirrored, back over two rows).  dword mode: consecutive lanes, consecutive addresses.
__device__ __forceinline__ void place_step(const TailSrcs& src, const TailGeom& g, float* tile, long t, int s, int k,
                                           const TailRegs& r) {
  const TileSpan ts = tile_span(g, t);
  const bool mirrored = src.flip[s] != 0;
  const bool first = s == 0;
  const int C = g.C, S = g.S;
  if (g.vec) {
    const SpanVecs sv = span_vecs(g, ts, mirrored ? ts.pm : ts.p0);
    const int delta = mirrored ? -(S + C) : S - C;
    const int rot = (threadIdx.x >> 3) & 3;
    const int dj = (4 * NT) / C, dc = 4 * NT - dj * C;
    int rel0 = sv.r00 + 4 * (k * 4 * NT + (int)threadIdx.x);
    PixCls pc = pix_cls(rel0, C);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if ((k * 4 + u) * NT + (int)threadIdx.x < sv.nvec) {
        const int base = (mirrored ? ts.n - 1 - pc.js : pc.js) * S + pc.c;
        const bool interior = rel0 >= 0 && rel0 + 3 < ts.nel;
        int a[4];
        float x[4], old[4];
        float f0 = r.f[4 * u], f1 = r.f[4 * u + 1], f2 = r.f[4 * u + 2], f3 = r.f[4 * u + 3];
        const long e = (sv.q0 + (k * 4 + u) * NT + (int)threadIdx.x) * 4;
        if (e + 4 > g.total) {                                   // the buffer's last, partial vector
          const float* __restrict__ sp = src.p[s];
          f0 = e < g.total ? sp[e] : 0.f;
          f1 = e + 1 < g.total ? sp[e + 1] : 0.f;
          f2 = e + 2 < g.total ? sp[e + 2] : 0.f;
          f3 = 0.f;
        }
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const int c4 = (kk + rot) & 3;
          x[kk] = pick4(c4, f0, f1, f2, f3);
          a[kk] = base + c4 + (pc.c + c4 >= C ? delta : 0);
          if (!(interior || (rel0 + c4 >= 0 && rel0 + c4 < ts.nel))) a[kk] = -1;
        }
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) old[kk] = (first || a[kk] < 0) ? 0.0f : tile[a[kk]];   // four reads in flight
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
          if (a[kk] >= 0) tile[a[kk]] = old[kk] + x[kk];
      }
      rel0 += 4 * NT;
      advance(pc, dj, dc, C);
    }
  } else {
    PixCls pc = pix_cls(k * 16 * NT + (int)threadIdx.x, C);
    const int dj = NT / C, dc = NT - dj * C;
#pragma unroll
    for (int m0 = 0; m0 < 16; m0 += 4) {
      int a[4];
      float old[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        a[m] = (k * 16 + m0 + m) * NT + (int)threadIdx.x < ts.nel ? (mirrored ? ts.n - 1 - pc.js : pc.js) * S + pc.c : -1;
        advance(pc, dj, dc, C);
      }
#pragma unroll
      for (int m = 0; m < 4; ++m) old[m] = (first || a[m] < 0) ? 0.0f : tile[a[m]];
#pragma unroll
      for (int m = 0; m < 4; ++m)
        if (a[m] >= 0) tile[a[m]] = old[m] + r.f[m0 + m];
    }
  }
}

__global__ __launch_bounds__(NT) void eval_tail_kernel(const TailSrcs src, const TailGeom g,
                                                       const int64_t* __restrict__ labels, int ignore_label,
                                                       float div_scales, float div_flips,
                                                       unsigned char* __restrict__ pred, float* __restrict__ prob,
                                                       unsigned char* __restrict__ err,
                                                       unsigned long long* __restrict__ hist,
                                                       double* __restrict__ loss_acc, float* __restrict__ avg,
                                                       int tile_floats) {
  SSA_DYN_LDS(float, tile);                                      // [seglen][S], then the histogram [C][C]
  unsigned int* lh = reinterpret_cast<unsigned int*>(tile + tile_floats);
  const int C = g.C, S = g.S, K = g.K;
  if (hist)
    for (int i = threadIdx.x; i < C * C; i += NT) lh[i] = 0u;    // (the first tile's barrier orders it)
  double lsum = 0.0, lcnt = 0.0;
  const bool divide = div_scales != 1.0f || div_flips != 1.0f;
  const long ntiles = g.rows * g.nseg;
  long t = blockIdx.x;                                           // the step being placed: (t, s, k)
  int s = 0, k = 0;
  long lab = -1;

  // One step: issue the loads of the step after this one into `nxt`, add `cur` into the tile; when that completes a
  // tile, the per-pixel pass.  Returns false after the workgroup's last step.
  auto step = [&](const TailRegs& cur, TailRegs& nxt) -> bool {
    long tn = t;
    int sn = s, kn = k + 1;
    if (kn == g.nchunk) { kn = 0; if (++sn == src.n) { sn = 0; tn += gridDim.x; } }
    if (tn < ntiles) issue_step(src, g, labels, tn, sn, kn, nxt);
    if (s && k == 0 && (src.flip[s] != 0) != (src.flip[s - 1] != 0)) __syncthreads();   // another thread owns the element
    if (s == 0 && k == 0) lab = cur.lab;
    place_step(src, g, tile, t, s, k, cur);
    if (tn != t) {                                               // the tile is complete
      const TileSpan ts = tile_span(g, t);
      __syncthreads();
      const int part = (int)threadIdx.x & (K - 1);
      const int j = (int)threadIdx.x / K;
      const bool owner = part == 0 && j < ts.n;
      float* x = tile + min(j, ts.n - 1) * S;
      float best = 0.f;
      int arg = C;
      const bool mine = j < ts.n;                                // (lanes past the segment only keep the exchanges whole)
      auto quotient = [&](float v) {
        v = g.rcp_scales != 0.f ? v * g.rcp_scales : v / div_scales;
        return g.rcp_flips != 0.f ? v * g.rcp_flips : v / div_flips;
      };
      auto first_max = [&](float v, int c) {                     // first maximum; NaN wins once
        if (arg == C || v > best || (v != v && best == best)) { best = v; arg = c; }
      };
      int c = part;
      for (; c + 3 * K < C; c += 4 * K) {                        // four LDS reads in flight
        float v0 = x[c], v1 = x[c + K], v2 = x[c + 2 * K], v3 = x[c + 3 * K];
        if (divide) {
          v0 = quotient(v0); v1 = quotient(v1); v2 = quotient(v2); v3 = quotient(v3);
          if (mine) { x[c] = v0; x[c + K] = v1; x[c + 2 * K] = v2; x[c + 3 * K] = v3; }
        }
        first_max(v0, c); first_max(v1, c + K); first_max(v2, c + 2 * K); first_max(v3, c + 3 * K);
      }
      for (; c < C; c += K) {
        float v = x[c];
        if (divide) { v = quotient(v); if (mine) x[c] = v; }
        first_max(v, c);
      }
      for (int o = 1; o < K; o <<= 1) {                          // the first maximum over the K lanes' class subsets
        const float ob = __shfl_xor(best, o, 64);
        const int oa = __shfl_xor(arg, o, 64);
        const bool bn = best != best, on = ob != ob;
        const bool take = oa < C && (arg == C || (on ? (!bn || oa < arg)
                                                     : (!bn && (ob > best || (ob == best && oa < arg)))));
        if (take) { best = ob; arg = oa; }
      }
      float se = 0.f;
      for (c = part; c + 3 * K < C; c += 4 * K) {
        const float e0 = __expf(x[c] - best), e1 = __expf(x[c + K] - best), e2 = __expf(x[c + 2 * K] - best),
                    e3 = __expf(x[c + 3 * K] - best);
        se += e0; se += e1; se += e2; se += e3;
      }
      for (; c < C; c += K) se += __expf(x[c] - best);
      for (int o = 1; o < K; o <<= 1) se += __shfl_xor(se, o, 64);
      ssa_wave_sync();                                           // x[gt] below may be another lane's quotient
      if (owner) {
        const long p = ts.p0 + j;
        const long gt = labels ? lab : -1L;
        if (pred) pred[p] = (unsigned char)arg;
        if (prob) prob[p] = 1.0f / se;
        if (err) err[p] = (gt >= 0 && gt != ignore_label && arg != gt) ? 1 : 0;
        const bool in_range = gt >= 0 && gt < C;
        if (hist && in_range) atomicAdd(&lh[(int)gt * C + arg], 1u);
        if (loss_acc && in_range && gt != ignore_label) {
          lsum += (double)((best + logf(se)) - x[gt]);
          lcnt += 1.0;
        }
      }
      __syncthreads();
      if (avg) {
        float* dst = avg + ts.p0 * C;                            // dense [P][C]
        for (int i = threadIdx.x; i < ts.nel; i += NT) {
          const int js = i / C;
          dst[i] = tile[js * S + (i - js * C)];
        }
        __syncthreads();
      }
    }
    t = tn; s = sn; k = kn;
    return t < ntiles;
  };

  TailRegs A, B;
  A.lab = B.lab = -1;
  if (t < ntiles) {
    issue_step(src, g, labels, t, 0, 0, A);
    while (step(A, B) && step(B, A)) {}
  }
  __syncthreads();
  if (hist)
    for (int i = threadIdx.x; i < C * C; i += NT)
      if (lh[i]) atomicAdd(&hist[i], (unsigned long long)lh[i]);
  if (loss_acc) ssa_block_acc2<NT>(lsum, lcnt, loss_acc);
}

inline float pow2_reciprocal(float d) {      // 1 / d if d is a power of two (x / d == x * (1 / d) exactly), else 0
  int e;
  return frexpf(d, &e) == 0.5f ? 1.0f / d : 0.f;
}

}  // namespace

extern "C" int ssa_eval_tail(const float* const* srcs, const int* flips, int n_src, int ld, int B, int H, int W, int C,
                             const int64_t* labels, int ignore_label, float div_scales, float div_flips,
                             unsigned char* pred, float* prob, unsigned char* err, int64_t* hist, double* loss_acc,
                             float* avg, void* stream) {
  if (!srcs || !flips || n_src < 1 || n_src > kMaxSrc || B < 1 || H < 1 || W < 1 || C < 1 || C > kMaxClasses || ld < C)
    return SSA_EINVAL;
  if (!(div_scales > 0.f) || !(div_flips > 0.f)) return SSA_EINVAL;
  if (!labels && (err || hist || loss_acc)) return SSA_EINVAL;
  if (!pred && !prob && !err && !hist && !loss_acc && !avg) return SSA_EINVAL;
  TailSrcs ts;
  TailGeom g;
  g.vec = ld == C && C >= 4 ? 1 : 0;
  for (int s = 0; s < kMaxSrc; ++s) {
    ts.p[s] = s < n_src ? srcs[s] : nullptr;
    ts.flip[s] = s < n_src ? (flips[s] != 0) : 0;
    if (s < n_src && !srcs[s]) return SSA_EINVAL;
    if (s < n_src && (reinterpret_cast<uintptr_t>(srcs[s]) & 15u)) g.vec = 0;
  }
  ts.n = n_src;
  const long P = (long)B * H * W;
  g.rows = (long)B * H;
  g.total = (P - 1) * ld + C;
  g.W = W; g.C = C; g.ld = ld;
  g.rcp_scales = pow2_reciprocal(div_scales);
  g.rcp_flips = pow2_reciprocal(div_flips);
  // segment length: the largest of 256 / 128 / 64 pixels whose tile + histogram stay within the budget, cut down to
  // what fills whole chunks of kChunkVecs float4 (one more vector than the span's floats / 4: the 16-byte grid)
  const size_t hist_bytes = hist ? (size_t)C * C * sizeof(unsigned int) : 0;
  int TP = 256;
  while (TP > 64 && (size_t)TP * (C + 4) * sizeof(float) + hist_bytes > kLdsBudget) TP >>= 1;
  g.nchunk = (TP * C / 4 + 1) / kChunkVecs;
  if (g.nchunk < 1) g.nchunk = 1;
  int cap = (g.nchunk * kChunkVecs - 1) * 4 / C;
  if (cap > TP) cap = TP;
  g.nseg = (W + cap - 1) / cap;
  g.seglen = (W + g.nseg - 1) / g.nseg;
  g.K = g.seglen * 4 <= NT ? 4 : g.seglen * 2 <= NT ? 2 : 1;
  g.S = (C + g.K - 1) / g.K * g.K;
  if (((g.S / g.K) & 1) == 0) g.S += g.K;
  const int tile_floats = g.seglen * g.S;
  const size_t lds = (size_t)tile_floats * sizeof(float) + hist_bytes;
  static ssa::LdsLimit lds_limit;           // per device (group.h)
  if (int rc = ssa::raise_lds_limit((const void*)eval_tail_kernel, lds, 64 * 1024, &lds_limit)) return rc;
  // persistent workgroups: every one ends in a histogram flush and two fp64 atomics, so no more of them than the chip
  // keeps resident (256 CUs x the workgroups per CU the LDS admits, at most four)
  long per_cu = (long)(160 * 1024 / lds);
  per_cu = per_cu < 1 ? 1 : per_cu > 4 ? 4 : per_cu;
  const long ntiles = g.rows * g.nseg;
  const int blocks = (int)(ntiles < 256 * per_cu ? ntiles : 256 * per_cu);
  hipLaunchKernelGGL(eval_tail_kernel, dim3(blocks), dim3(NT), lds, (hipStream_t)stream, ts, g, labels, ignore_label,
                     div_scales, div_flips, pred, prob, err, (unsigned long long*)hist, loss_acc, avg, tile_floats);
  SSA_LAUNCH_CHECK();
  return SSA_OK;
}
