// Constant padding of the (image, labels) pair on the device: what `ImageOps.expand(img, border, fill)` and add_margin
// (transforms/joint_transforms.py:48-60, 126-141, 173-177) produce for RGB and L images when RandomCrop meets an image
// smaller than the crop.  A copy: uint8 [H][W][channels] into the middle of [H+top+bottom][W+left+right][channels], the
// frame filled with `fill`.  One thread per output pixel.
#include "common.h"

namespace {

constexpr int NT = 256;

__global__ __launch_bounds__(NT) void pad_u8_kernel(const unsigned char* __restrict__ src, int H, int W, int ch, int left,
                                                    int top, int Hd, int Wd, unsigned f0, unsigned f1, unsigned f2,
                                                    unsigned char* __restrict__ dst) {
  const long n = (long)Hd * Wd;
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < n; i += (long)gridDim.x * NT) {
    const int y = (int)(i / Wd) - top, x = (int)(i % Wd) - left;
    const bool in = y >= 0 && y < H && x >= 0 && x < W;
    const unsigned char* p = src + ((long)(in ? y : 0) * W + (in ? x : 0)) * ch;
    if (ch == 1) {
      dst[i] = in ? p[0] : (unsigned char)f0;
    } else {
      dst[i * 3 + 0] = in ? p[0] : (unsigned char)f0;
      dst[i * 3 + 1] = in ? p[1] : (unsigned char)f1;
      dst[i * 3 + 2] = in ? p[2] : (unsigned char)f2;
    }
  }
}

}  // namespace

extern "C" {

int ssa_pad_u8(const unsigned char* src, int H, int W, int channels, int left, int top, int right, int bottom,
               const unsigned char* fill, unsigned char* dst, void* stream) {
  if (!src || !dst || !fill || H <= 0 || W <= 0 || (channels != 1 && channels != 3) || left < 0 || top < 0 || right < 0 ||
      bottom < 0)
    return SSA_EINVAL;
  const long Hd = (long)H + top + bottom, Wd = (long)W + left + right;
  if (Hd > 0x7fffffffL || Wd > 0x7fffffffL) return SSA_EINVAL;
  const long blocks = (Hd * Wd + NT - 1) / NT;
  hipLaunchKernelGGL(pad_u8_kernel, dim3((int)(blocks > 16384 ? 16384 : blocks)), dim3(NT), 0, (hipStream_t)stream, src, H,
                     W, channels, left, top, (int)Hd, (int)Wd, (unsigned)fill[0], (unsigned)fill[1],
                     (unsigned)fill[2], dst);
  SSA_LAUNCH_CHECK();
  return SSA_OK;
}

}  // extern "C"
