// Evaluation-time visualisation (eval_config.num_visualizations): rectangle outlines painted into a uint8 image on the
// device. Declared in include/mtlssl_hip.h (mtlssl_draw_boxes).
#include "common.h"

using namespace mtlssl;

namespace {

// One thread per pixel. Boxes are painted in input order, i.e. the LAST box whose outline covers the pixel decides its
// colour: scan from the last box to the first and stop at the first hit. The box table is read at wave-uniform
// addresses (every lane the same box), the pixel is written with three byte stores; a pixel no outline covers is
// neither read nor written.
__global__ void __launch_bounds__(256)
    k_draw_boxes(uint8_t* image, int H, int W, int64_t row_stride, const int32_t* boxes, const uint8_t* colors,
                 int n, int thickness) {
  int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= (int64_t)H * W) return;
  int y = (int)(p / W), x = (int)(p % W);
  for (int i = n - 1; i >= 0; --i) {
    int y0 = boxes[4 * i + 0], x0 = boxes[4 * i + 1], y1 = boxes[4 * i + 2], x1 = boxes[4 * i + 3];
    if (y < y0 || y >= y1 || x < x0 || x >= x1) continue;          // outside [y0,y1) x [x0,x1) (empty when degenerate)
    // int64: y0 + thickness of a box far outside the image must not wrap
    bool inner = y >= (int64_t)y0 + thickness && y < (int64_t)y1 - thickness && x >= (int64_t)x0 + thickness &&
                 x < (int64_t)x1 - thickness;
    if (inner) continue;
    uint8_t* px = image + (int64_t)y * row_stride + (int64_t)x * 3;
    px[0] = colors[3 * i + 0];
    px[1] = colors[3 * i + 1];
    px[2] = colors[3 * i + 2];
    return;
  }
}

}  // namespace

extern "C" int mtlssl_draw_boxes(uint8_t* image, int height, int width, int64_t row_stride, const int32_t* boxes,
                                 const uint8_t* colors, int n, int thickness, mtlssl_stream_t stream) {
  MTLSSL_REQUIRE(height >= 0 && width >= 0 && n >= 0, "draw_boxes: negative size");
  MTLSSL_REQUIRE(row_stride >= (int64_t)width * 3, "draw_boxes: row_stride %lld < 3 * width %d", (long long)row_stride,
                 width);
  MTLSSL_REQUIRE(thickness >= 1, "draw_boxes: thickness %d < 1", thickness);
  int64_t pixels = (int64_t)height * width;
  if (!pixels || !n) return MTLSSL_OK;
  MTLSSL_REQUIRE(image && boxes && colors, "draw_boxes: null pointer");
  MTLSSL_REQUIRE(cdiv(pixels, 256) <= 0x7fffffff, "draw_boxes: image too large");
  hipLaunchKernelGGL(k_draw_boxes, dim3((unsigned)cdiv(pixels, 256)), dim3(256), 0, S(stream), image, height, width,
                     row_stride, boxes, colors, n, thickness);
  return check_launch("draw_boxes");
}
