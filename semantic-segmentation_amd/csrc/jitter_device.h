// The per-pixel steps of the device ColorJitter, shared by color_jitter.hip (which states the arithmetic) and gblur.hip
// (which runs them on every pixel it stages): Pillow's luma, Image.blend, the HSV round trip of adjust_hue, the
// program interpreter and the contrast mean read from the luma counter, plus the host-side check of a program (the
// streaming kernel that runs them is in input_tail.h).  Every product and sum is rounded on its own (see color_jitter.hip): the functions that multiply and add
// carry the pragma themselves, so they stay uncontracted whatever the including file is compiled under.
#pragma once
#include <cmath>
#include "common.h"
#include "../../include/semseg_hip.h"

namespace {

__device__ __forceinline__ int luma(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

// Image.blend(degenerate, img, f) of one channel
__device__ __forceinline__ int blend(int d, int x, float f, bool clip) {
#pragma clang fp contract(off)
  const float t = (float)d + f * ((float)x - (float)d);
  if (clip) {
    if (t <= 0.f) return 0;
    if (t >= 255.f) return 255;
  }
  return (int)t;
}

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// rgb2hsv + (H + shift) mod 256 + hsv2rgb of libImaging/Convert.c
__device__ __forceinline__ void hue_shift(int& r, int& g, int& b, int shift) {
#pragma clang fp contract(off)
  const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
  if (maxc == minc) return;                       // S == 0: grey V whatever H is
  const float cr = (float)(maxc - minc);
  const float s = __fdiv_rn(cr, (float)maxc);
  const float rc = __fdiv_rn((float)(maxc - r), cr), gc = __fdiv_rn((float)(maxc - g), cr),
              bc = __fdiv_rn((float)(maxc - b), cr);
  float h;
  if (r == maxc) h = bc - gc;
  else if (g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
  else h = (float)(4.0 + (double)gc - (double)rc);
  double hd = (double)h / 6.0 + 1.0;              // in [5/6, 11/6]; fmod(hd, 1.0) is this exact subtraction
  if (hd >= 1.0) hd -= 1.0;
  h = (float)hd;
  const int H = (clip8((int)((double)h * 255.0)) + shift) & 255;
  const int S = clip8((int)((double)s * 255.0)), V = maxc;
  if (S == 0) { r = g = b = V; return; }
  const double hf = (double)H * 6.0 / 255.0;
  const int i = (int)floor(hf);
  const double f = hf - (double)i, fs = (double)S / 255.0, v = (double)V;
  const int p = clip8((int)floor(v * (1.0 - fs) + 0.5));
  const int q = clip8((int)floor(v * (1.0 - fs * f) + 0.5));
  const int t = clip8((int)floor(v * (1.0 - fs * (1.0 - f)) + 0.5));
  switch (i % 6) {
    case 0: r = V; g = t; b = p; break;
    case 1: r = q; g = V; b = p; break;
    case 2: r = p; g = V; b = t; break;
    case 3: r = p; g = q; b = V; break;
    case 4: r = t; g = p; b = V; break;
    default: r = V; g = p; b = q; break;
  }
}

__device__ __forceinline__ bool blend_clips(float f) { return !(f >= 0.f && f <= 1.f); }

// One step of the program on one pixel (m: the contrast mean; unused by the other steps)
__device__ __forceinline__ void jitter_step(const ssa_jitter_program& pg, int op, int m, int& r, int& g, int& b) {
  if (op == SSA_JITTER_HUE) {
    hue_shift(r, g, b, pg.hue_byte);
    return;
  }
  const float f = pg.factor[op];
  const bool clip = blend_clips(f);
  if (op == SSA_JITTER_SATURATION) m = luma(r, g, b);
  else if (op == SSA_JITTER_BRIGHTNESS) m = 0;
  r = blend(m, r, f, clip);
  g = blend(m, g, f, clip);
  b = blend(m, b, f, clip);
}

// The steps in front of the (first) contrast step, then L: what ImageEnhance.Contrast averages
__device__ __forceinline__ int jitter_luma_before_contrast(const ssa_jitter_program& pg, int r, int g, int b) {
  for (int k = 0; k < pg.n_ops && pg.op[k] != SSA_JITTER_CONTRAST; ++k) jitter_step(pg, pg.op[k], 0, r, g, b);
  return luma(r, g, b);
}

__device__ __forceinline__ void jitter_pixel(const ssa_jitter_program& pg, int m, int& r, int& g, int& b) {
  for (int k = 0; k < pg.n_ops; ++k) jitter_step(pg, pg.op[k], m, r, g, b);
}

// m = int(S / N + 0.5) with the division in double (ImageStat.Stat(...).mean[0] + 0.5, truncated)
__device__ __forceinline__ int contrast_mean(const ssa_jitter_program& pg, const unsigned long long* counter, long n) {
  for (int k = 0; k < pg.n_ops; ++k)
    if (pg.op[k] == SSA_JITTER_CONTRAST) return (int)((double)*counter / (double)n + 0.5);
  return 0;
}

// 0..4 distinct known op codes and finite factors (blend converts f * (x - d) + d to int: undefined for NaN and infinity);
// *has_contrast tells whether the program needs the luma sum
bool program_ok(const ssa_jitter_program* pg, bool* has_contrast) {
  if (!pg || pg->n_ops < 0 || pg->n_ops > 4 || pg->hue_byte < 0 || pg->hue_byte > 255) return false;
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(pg->factor[k])) return false;
  unsigned seen = 0;
  for (int k = 0; k < pg->n_ops; ++k) {
    const int op = pg->op[k];
    if (op < SSA_JITTER_BRIGHTNESS || op > SSA_JITTER_HUE || (seen >> op & 1u)) return false;
    seen |= 1u << op;
  }
  *has_contrast = seen >> SSA_JITTER_CONTRAST & 1u;
  return true;
}

}  // namespace
