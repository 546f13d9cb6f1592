// Host-side checks of the scene entry points (scene.hip, conv_valu.hip), one per property of the window table.  They read the HOST copy
// of the table, which the kernels rely on having been checked.  `who`: the entry point, prefix of every message.  SC_OK or SC_ERR_ARG.
#pragma once
#include "sc_common.h"

// sc_scene_gather / sc_scene_gather_planes: n windows of win_h x win_w out of the reflect-padded H x W scene
inline int sc_scene_check_gather(const char* who, int H, int W, int pad_top, int pad_left, int n, int win_h, int win_w, const void* out,
                                 const sc_scene_win* win, const sc_scene_win* win_host) {
  SC_REQUIRE(pad_top >= 0 && pad_top < H && pad_left >= 0 && pad_left < W,
             "%s: reflect padding (%d, %d) needs the image (%d x %d) to be larger than the pad", who, pad_top, pad_left, H, W);
  SC_REQUIRE(n >= 1 && n <= (1 << 20), "%s: n=%d outside [1, 2^20]", who, n);
  SC_REQUIRE(win_h >= 1 && win_w >= 4 && win_w % 4 == 0 && (long long)win_h * win_w < (1ll << 31),
             "%s: bad window size %d x %d (the width must be a multiple of 4)", who, win_h, win_w);
  SC_REQUIRE((uintptr_t)out % 16 == 0 && (uintptr_t)win % 4 == 0, "%s: misaligned output or window table", who);
  for (int i = 0; i < n; ++i) {
    const sc_scene_win& q = win_host[i];
    // one reflection: rows -pad_top .. 2H - 2 - pad_top of the padded scene exist, i.e. the bottom / right pad is below H / W too
    SC_REQUIRE(q.row_off >= 0 && q.col_off >= 0 && (long long)q.row_off + win_h - pad_top <= 2ll * H - 1 && (long long)q.col_off + win_w - pad_left <= 2ll * W - 1,
               "%s: window %d (row %d, col %d, %d x %d) leaves the reflect-padded scene (pads must stay below the image size)", who, i,
               q.row_off, q.col_off, win_h, win_w);
  }
  return SC_OK;
}

// the mosaic heads: the cores of N windows of an H x W plane go into a mos_h x mos_w mosaic; an empty core stores nothing
inline int sc_scene_check_cores(const char* who, const sc_scene_win* win_host, int N, int H, int W, int mos_h, int mos_w) {
  for (int i = 0; i < N; ++i) {
    const sc_scene_win& q = win_host[i];
    if (q.core_y1 <= q.core_y0 || q.core_x1 <= q.core_x0) continue;
    SC_REQUIRE(q.core_y0 >= 0 && q.core_y1 <= H && q.core_x0 >= 0 && q.core_x1 <= W,
               "%s: core %d (rows %d:%d, columns %d:%d) is not inside the %d x %d plane", who, i, q.core_y0, q.core_y1, q.core_x0, q.core_x1, H, W);
    SC_REQUIRE(q.dst_row >= 0 && (long long)q.dst_row + (q.core_y1 - q.core_y0) <= mos_h && q.dst_col >= 0 && (long long)q.dst_col + (q.core_x1 - q.core_x0) <= mos_w,
               "%s: core %d does not fit the %d x %d mosaic at row %d, column %d", who, i, mos_h, mos_w, q.dst_row, q.dst_col);
  }
  return SC_OK;
}
