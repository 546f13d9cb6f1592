// Validation panels (starcop/plot.py plot_batch; starcop/validation.py:137-153): the image panels of a products_plot figure, drawn
// straight into PNG scanlines on the device.  The per-pixel arithmetic is the contract in include/starcop_hip.h; keep this file free
// of fast-math flags, the BAND path relies on the correctly rounded float32 division hipcc emits by default.
//
// sc_render_panels, one launch, grid = (blocks, n_panels + 1):
//   y < n_panels  a work-group owns one source row x one chunk of PN_CW canvas columns of panel y (grid.x is sized for the panel with
//                 the most work-groups; the surplus of the others exits at once).  Lanes along x load the source pixels of the chunk
//                 once (coalesced) and leave their packed colours in LDS; the row segment (3 bytes per canvas pixel, every source
//                 colour `scale` times) is assembled in LDS as 4-byte words; then it is copied to each of the `scale` canvas rows.  The pitch 1 + 3 Wc leaves canvas rows at any alignment, so every copy re-aligns: byte
//                 stores up to the first 4-byte boundary, aligned word stores (two LDS words funnel-shifted into one), byte stores
//                 for the ragged tail.  Consecutive lanes store consecutive words.
//   y == n_panels the background: a work-group owns one canvas row, lists the panels that cross it in LDS and writes what
//                 no panel covers -- the filter byte (0) and white gap pixels -- as aligned words where a whole word is background,
//                 byte by byte where a word is shared with a panel.
//   No byte is written twice, so there is nothing to order; no atomics on memory, no workspace.  The kernel trusts the device table
//   for source addresses only: a destination outside the canvas is skipped, whatever the table holds.
// sc_panel_minmax: one work-group of 1024 threads per panel, waves along rows, lanes along x; min/max are order-independent.
#include <limits.h>
#include <math.h>

#include "sc_common.h"

namespace {

constexpr int PN_WG = 256;
constexpr int PN_CW = 1024;        // canvas pixels per chunk: 3 KiB of scanline
constexpr int PN_MM_WG = 1024;

// (viridis.colors * 255).astype(uint8) of matplotlib, generated from ../data/viridis8.txt by the Makefile
__device__ const unsigned char k_viridis8[768] = {
#include "viridis8.inc"
};

struct RenderD {
  const sc_panel* tab;
  const float* mm;
  unsigned char* canvas;
  int n, Hc, Wc;
};

__device__ __forceinline__ float pn_load(const void* p, int dtype, long long i) {
  if (dtype == SC_PANEL_F32) return static_cast<const float*>(p)[i];
  if (dtype == SC_PANEL_I64) return (float)static_cast<const long long*>(p)[i];
  return (float)static_cast<const unsigned char*>(p)[i];
}

__device__ __forceinline__ bool pn_finite(float v) { return fabsf(v) <= 3.4028234663852886e38f; }   // false for NaN

constexpr unsigned PN_WHITE = 0x00FFFFFFu;

// packed colour r | g << 8 | b << 16 of source pixel i of a panel
__device__ __forceinline__ unsigned pn_colour(const sc_panel& p, long long i, float vmin, float d, bool flat, const unsigned* lut) {
  if (p.kind == SC_PANEL_BAND) {
    float v = pn_load(p.src[0], p.dtype, i);
    if (p.div != 1.0f) v = v / p.div;
    if (!pn_finite(v)) return PN_WHITE;
    const float t = flat ? 0.0f : (v - vmin) / d;
    const float xa = t * 256.0f;
    const int idx = xa < 0.0f ? 0 : (xa >= 256.0f ? 255 : (int)xa);
    return lut[idx];
  }
  if (p.kind == SC_PANEL_RGB) {
    unsigned out = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float v = pn_load(p.src[c], p.dtype, i);
      if (v != v) return PN_WHITE;
      const float cl = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
      out |= (unsigned)(int)(cl * 255.0f) << (8 * c);
    }
    return out;
  }
  const float v = pn_load(p.src[0], p.dtype, i);
  unsigned out = 0;
#pragma unroll
  for (int k = 0; k < SC_PANEL_MAX_CAT; ++k)
    if (k < p.n_cat && v == p.cat_value[k]) out = (unsigned)p.cat_rgb[k][0] | (unsigned)p.cat_rgb[k][1] << 8 | (unsigned)p.cat_rgb[k][2] << 16;
  return out;
}

// copies n bytes of the LDS segment `seg` (word array, one word of padding behind the data) to global `g`, any alignment
__device__ __forceinline__ void pn_store_segment(unsigned char* g, const unsigned* seg, int n) {
  const unsigned char* segb = reinterpret_cast<const unsigned char*>(seg);
  int head = (int)((4u - (unsigned)(reinterpret_cast<uintptr_t>(g) & 3u)) & 3u);
  if (head > n) head = n;
  const int nw = (n - head) >> 2;
  const int tail0 = head + 4 * nw;
  if ((int)threadIdx.x < head) g[threadIdx.x] = segb[threadIdx.x];
  unsigned* gw = reinterpret_cast<unsigned*>(g + head);
  const int sh = 8 * head;                       // head in 0..3: word i starts at segment byte head + 4 i
  for (int i = threadIdx.x; i < nw; i += PN_WG) {
    const unsigned long long two = (unsigned long long)seg[i + 1] << 32 | seg[i];
    gw[i] = (unsigned)(two >> sh);
  }
  const int t = (int)threadIdx.x - (PN_WG - 4);  // the last lanes take the tail, away from the head's
  if (t >= 0 && tail0 + t < n) g[tail0 + t] = segb[tail0 + t];
}

__global__ __launch_bounds__(PN_WG) void k_render_panels(const RenderD a) {
  __shared__ unsigned lut[256];
  __shared__ unsigned col[PN_CW];                          // packed colours of the chunk's source pixels
  __shared__ unsigned seg[3 * PN_CW / 4 + 1];              // the assembled row segment
  __shared__ int bg_x0[SC_PANEL_MAX], bg_x1[SC_PANEL_MAX]; // background: pixel ranges of the panels crossing the row
  __shared__ int bg_n;
  const size_t pitch = 1 + 3 * (size_t)a.Wc;

  if ((int)blockIdx.y < a.n) {
    const sc_panel p = a.tab[blockIdx.y];
    const long long wpx_full = (long long)p.W * p.scale;
    if (p.scale < 1 || p.H < 1 || p.W < 1 || p.dst_x < 0 || p.dst_y < 0 || p.dst_x + wpx_full > a.Wc) return;
    const int wpx = (int)wpx_full;                         // canvas pixels per panel row (<= Wc)
    const unsigned chunks = (unsigned)((wpx + PN_CW - 1) / PN_CW);
    if (blockIdx.x >= chunks * (unsigned)p.H) return;      // the grid is sized for the panel with the most work-groups
    const unsigned yu = blockIdx.x / chunks, cx = blockIdx.x - yu * chunks;
    const int y = (int)yu;
    const int px0 = (int)cx * PN_CW, px1 = min(wpx, px0 + PN_CW);
    const int sx0 = px0 / p.scale, ns = (px1 - 1) / p.scale + 1 - sx0;         // source pixels of the chunk (<= PN_CW)
    const int nbytes = 3 * (px1 - px0);
    lut[threadIdx.x] = (unsigned)k_viridis8[3 * threadIdx.x] | (unsigned)k_viridis8[3 * threadIdx.x + 1] << 8 |
                       (unsigned)k_viridis8[3 * threadIdx.x + 2] << 16;
    float vmin = p.vmin, vmax = p.vmax;
    if (p.autoscale && a.mm) { vmin = a.mm[2 * blockIdx.y]; vmax = a.mm[2 * blockIdx.y + 1]; }
    const float d = (float)((double)vmax - (double)vmin);
    const bool flat = vmax == vmin;
    __syncthreads();                                       // the lut is in place
    const long long row = (long long)y * p.row_stride + sx0;
    for (int i = threadIdx.x; i < ns; i += PN_WG) col[i] = pn_colour(p, row + i, vmin, d, flat, lut);
    __syncthreads();
    for (int j = threadIdx.x; 4 * j < nbytes; j += PN_WG) {
      unsigned w = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int k = 4 * j + b, q = k / 3, ch = k - 3 * q;
        int si = p.scale == 1 ? q : (int)((unsigned)(px0 + q) / (unsigned)p.scale) - sx0;
        si = min(si, ns - 1);                              // the bytes of the last word behind the segment
        w |= ((col[si] >> (8 * ch)) & 255u) << (8 * b);
      }
      seg[j] = w;
    }
    if (threadIdx.x == 0) seg[(nbytes + 3) / 4] = 0;       // the word the funnel shift reads behind the data
    __syncthreads();
    for (int s = 0; s < p.scale; ++s) {
      const long long Y = (long long)p.dst_y + (long long)y * p.scale + s;
      if (Y >= a.Hc) break;
      pn_store_segment(a.canvas + (size_t)Y * pitch + 1 + 3 * ((size_t)p.dst_x + px0), seg, nbytes);
    }
    return;
  }

  // ---- background: canvas row blockIdx.x ----
  const long long Y = blockIdx.x;
  if (Y >= a.Hc) return;                                   // uniform
  if (threadIdx.x == 0) bg_n = 0;
  __syncthreads();
  for (int i = threadIdx.x; i < a.n && i < SC_PANEL_MAX; i += PN_WG) {
    const sc_panel& p = a.tab[i];
    const long long y0 = p.dst_y, yend = y0 + (long long)p.H * p.scale;
    if (Y >= y0 && Y < yend) {
      const int at = atomicAdd(&bg_n, 1);                  // LDS; the order of the list does not matter
      bg_x0[at] = p.dst_x;
      bg_x1[at] = (int)min((long long)a.Wc, p.dst_x + (long long)p.W * p.scale);
    }
  }
  __syncthreads();
  const int nl = bg_n;
  unsigned char* g = a.canvas + (size_t)Y * pitch;
  const int n = (int)pitch;
  const int head = (int)((4u - (unsigned)(reinterpret_cast<uintptr_t>(g) & 3u)) & 3u);
  // word index i covers row bytes head + 4 (i - 1) .. + 3; i = 0 is the (partial) head word
  for (int i = threadIdx.x; head + 4 * (i - 1) < n; i += PN_WG) {
    const int k0 = head + 4 * (i - 1);
    unsigned w = 0, bgmask = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int k = k0 + b;
      if (k < 0 || k >= n) continue;
      bool covered = false;
      unsigned val = 0;                                    // the filter byte
      if (k > 0) {
        const int q = (k - 1) / 3;
        val = 255u;
        for (int l = 0; l < nl; ++l) covered |= (q >= bg_x0[l] && q < bg_x1[l]);
      }
      if (!covered) { bgmask |= 1u << b; w |= val << (8 * b); }
    }
    if (bgmask == 0xFu) {
      *reinterpret_cast<unsigned*>(g + k0) = w;
    } else {
#pragma unroll
      for (int b = 0; b < 4; ++b)
        if (bgmask & (1u << b)) g[k0 + b] = (unsigned char)(w >> (8 * b));
    }
  }
}

__global__ __launch_bounds__(PN_MM_WG) void k_panel_minmax(const sc_panel* tab, float* out) {
  __shared__ float s_lo[PN_MM_WG / 64], s_hi[PN_MM_WG / 64];
  const sc_panel p = tab[blockIdx.x];
  if (!p.autoscale) {
    if (threadIdx.x == 0) { out[2 * blockIdx.x] = p.vmin; out[2 * blockIdx.x + 1] = p.vmax; }
    return;
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float lo = __builtin_inff(), hi = -__builtin_inff();
  for (int y = wave; y < p.H; y += PN_MM_WG / 64) {
    const long long row = (long long)y * p.row_stride;
    for (int x = lane; x < p.W; x += 64) {
      float v = pn_load(p.src[0], p.dtype, row + x);
      if (p.div != 1.0f) v = v / p.div;
      if (pn_finite(v)) { lo = fminf(lo, v); hi = fmaxf(hi, v); }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, o, 64));
    hi = fmaxf(hi, __shfl_xor(hi, o, 64));
  }
  if (lane == 0) { s_lo[wave] = lo; s_hi[wave] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < PN_MM_WG / 64; ++w) { lo = fminf(lo, s_lo[w]); hi = fmaxf(hi, s_hi[w]); }
    const bool none = lo > hi;
    out[2 * blockIdx.x] = none ? 0.0f : lo;
    out[2 * blockIdx.x + 1] = none ? 1.0f : hi;
  }
}

// the checks both entry points share; canvas_h < 0: no canvas (sc_panel_minmax)
int pn_check_table(const char* who, const sc_panel* dev, const sc_panel* t, int n, int canvas_h, int canvas_w) {
  SC_REQUIRE(dev && t, "%s: null panel table", who);
  SC_REQUIRE(n >= 1 && n <= SC_PANEL_MAX, "%s: n_panels=%d outside [1, %d]", who, n, SC_PANEL_MAX);
  SC_REQUIRE((uintptr_t)dev % 8 == 0, "%s: misaligned device table", who);
  for (int i = 0; i < n; ++i) {
    const sc_panel& p = t[i];
    SC_REQUIRE(p.dtype == SC_PANEL_F32 || p.dtype == SC_PANEL_I64 || p.dtype == SC_PANEL_U8, "%s: panel %d: unknown dtype %d", who, i, p.dtype);
    SC_REQUIRE(p.kind == SC_PANEL_BAND || p.kind == SC_PANEL_RGB || p.kind == SC_PANEL_CATEGORICAL, "%s: panel %d: unknown kind %d", who, i, p.kind);
    SC_REQUIRE(p.scale >= 1, "%s: panel %d: scale %d < 1", who, i, p.scale);
    SC_REQUIRE(p.H >= 1 && p.W >= 1 && p.row_stride >= p.W, "%s: panel %d: bad plane %d x %d, row stride %lld", who, i, p.H, p.W,
               (long long)p.row_stride);
    const int elem = p.dtype == SC_PANEL_F32 ? 4 : (p.dtype == SC_PANEL_I64 ? 8 : 1);
    for (int c = 0; c < (p.kind == SC_PANEL_RGB ? 3 : 1); ++c)
      SC_REQUIRE(p.src[c] && (uintptr_t)p.src[c] % elem == 0, "%s: panel %d: null or misaligned source plane %d", who, i, c);
    SC_REQUIRE(!p.autoscale || p.kind == SC_PANEL_BAND, "%s: panel %d: autoscale on a panel that is not a BAND", who, i);
    SC_REQUIRE(isfinite(p.div) && p.div != 0.0f, "%s: panel %d: divisor %g", who, i, (double)p.div);
    SC_REQUIRE(p.kind != SC_PANEL_BAND || p.autoscale || (isfinite(p.vmin) && isfinite(p.vmax)), "%s: panel %d: limits (%g, %g) are not finite",
               who, i, (double)p.vmin, (double)p.vmax);
    SC_REQUIRE(p.n_cat >= 0 && p.n_cat <= SC_PANEL_MAX_CAT, "%s: panel %d: n_cat=%d outside [0, %d]", who, i, p.n_cat, SC_PANEL_MAX_CAT);
    if (canvas_h < 0) continue;
    SC_REQUIRE(p.dst_y >= 0 && p.dst_x >= 0 && p.dst_y + (long long)p.H * p.scale <= canvas_h && p.dst_x + (long long)p.W * p.scale <= canvas_w,
               "%s: panel %d: rectangle (%d, %d) + %lld x %lld leaves the %d x %d canvas", who, i, p.dst_y, p.dst_x, (long long)p.H * p.scale,
               (long long)p.W * p.scale, canvas_h, canvas_w);
    for (int j = 0; j < i; ++j) {
      const sc_panel& q = t[j];
      const bool apart = p.dst_y + (long long)p.H * p.scale <= q.dst_y || q.dst_y + (long long)q.H * q.scale <= p.dst_y ||
                         p.dst_x + (long long)p.W * p.scale <= q.dst_x || q.dst_x + (long long)q.W * q.scale <= p.dst_x;
      SC_REQUIRE(apart, "%s: panels %d and %d overlap", who, j, i);
    }
  }
  return SC_OK;
}

}  // namespace

extern "C" int sc_panel_minmax(const sc_panel* table_dev, const sc_panel* table_host, int n_panels, float* out_minmax_dev, sc_stream stream) {
  const int rc = pn_check_table("sc_panel_minmax", table_dev, table_host, n_panels, -1, -1);
  if (rc != SC_OK) return rc;
  SC_REQUIRE(out_minmax_dev && (uintptr_t)out_minmax_dev % 4 == 0, "sc_panel_minmax: null or misaligned output");
  hipLaunchKernelGGL(k_panel_minmax, dim3((unsigned)n_panels), dim3(PN_MM_WG), 0, (hipStream_t)stream, table_dev, out_minmax_dev);
  SC_LAUNCH_OK("sc_panel_minmax");
  return SC_OK;
}

extern "C" int sc_render_panels(const sc_panel* table_dev, const sc_panel* table_host, int n_panels, const float* minmax_dev,
                                uint8_t* canvas, int canvas_h, int canvas_w, sc_stream stream) {
  SC_REQUIRE(canvas, "sc_render_panels: null canvas");
  SC_REQUIRE(canvas_h >= 1 && canvas_w >= 1 && canvas_w <= (INT_MAX - 1) / 3, "sc_render_panels: bad canvas %d x %d", canvas_h, canvas_w);
  const int rc = pn_check_table("sc_render_panels", table_dev, table_host, n_panels, canvas_h, canvas_w);
  if (rc != SC_OK) return rc;
  long long blocks = canvas_h;                             // grid.x: the background's rows or the panel with the most work-groups
  bool any_auto = false;
  for (int i = 0; i < n_panels; ++i) {
    const sc_panel& p = table_host[i];
    const long long b = (((long long)p.W * p.scale + PN_CW - 1) / PN_CW) * p.H;
    if (b > blocks) blocks = b;
    any_auto |= p.autoscale != 0;
  }
  SC_REQUIRE(!any_auto || (minmax_dev && (uintptr_t)minmax_dev % 4 == 0), "sc_render_panels: an autoscale panel needs minmax_dev");
  SC_REQUIRE(blocks <= INT_MAX, "sc_render_panels: grid of %lld work-groups is too large for one launch", blocks);
  RenderD d;
  d.tab = table_dev; d.mm = minmax_dev; d.canvas = canvas; d.n = n_panels; d.Hc = canvas_h; d.Wc = canvas_w;
  hipLaunchKernelGGL(k_render_panels, dim3((unsigned)blocks, (unsigned)n_panels + 1), dim3(PN_WG), 0, (hipStream_t)stream, d);
  SC_LAUNCH_OK("sc_render_panels");
  return SC_OK;
}
