// TEST-ONLY: the tile walk of the camera kernels (fly::render_strip, peg_in_hole_gym_amd/csrc/pih_fly_render.h) on the host, for the host
// builds of the cameras: the whole image, no strips, the same 16 x 64 tiles in the same order; the lane loop stands for the ballot.
// Include after the scene's product header.
#pragma once
#include <stddef.h>

namespace pih {

// px(prims, xc, yc, index of the pixel in the image) for every pixel; prims = the tile's primitive list: the product's screen-bound test
// (cull != 0; lanes past the scene's primitives are off), or `all_prims` for every tile
template <class MASK, class S, class PX> void host_tiles(const S& sc, int W, int H, int cull, MASK all_prims, PX&& px) {
  using fly::TILE_COLS; using fly::TILE_ROWS;
  const fly::FlyGrid g(sc, W, H);
  const int tcols = (W + TILE_COLS - 1) / TILE_COLS, trows = (H + TILE_ROWS - 1) / TILE_ROWS;
  for (int tile = 0; tile < tcols * trows; tile++) {
    const int ti = tile / tcols, tj = tile - ti * tcols;
    const int i0 = ti * TILE_ROWS, i1 = i0 + TILE_ROWS < H ? i0 + TILE_ROWS : H, j0 = tj * TILE_COLS, j1 = j0 + TILE_COLS < W ? j0 + TILE_COLS : W;
    MASK prims = all_prims;
    if (cull) {
      prims = 0;
      for (int lane = 0; lane < (int)(8 * sizeof(MASK)); lane++)
        if (prim_on_tile(sc, lane, g.xedge(j0), g.xedge(j1), g.yedge(i1), g.yedge(i0))) prims |= (MASK)1 << lane;
    }
    for (int i = i0; i < i1; i++)
      for (int j = j0; j < j1; j++) px(prims, g.xc(j), g.yc(i), (size_t)i * W + j);
  }
}

// one pixel into the output arrays of the pih*_render functions, each of which may be NULL: out double[H][W][4] = depth, r, g, b;
// rgba uint8[H][W][4] = r, g, b, seg; depth double[H][W].  `p` has the pixel's three formats (fly::Pixels, lit::LitPixels)
template <class MASK, class P> void host_store(const P& p, MASK prims, real xc, real yc, size_t px, double* out, unsigned char* rgba, double* depth) {
  if (out) {
    const real4 c = p.as_float4(prims, xc, yc);
    double* o = out + px * 4;
    o[0] = (double)c.x; o[1] = (double)c.y; o[2] = (double)c.z; o[3] = (double)c.w;
  }
  if (rgba) {
    const unsigned v = p.as_rgba8(prims, xc, yc);
    for (int k = 0; k < 4; k++) rgba[4 * px + k] = (unsigned char)((v >> (8 * k)) & 255u);
  }
  if (depth) depth[px] = (double)p.as_depth(prims, xc, yc);
}

}  // namespace pih
