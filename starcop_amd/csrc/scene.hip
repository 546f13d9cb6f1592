// Whole-scene cloud masking (starcop/sentinel2/models.py:27-52, 80-89: padded_predict reflect-pads the scene to a multiple of 32 and
// runs it as one image).  sc_scene_gather cuts n equally shaped windows out of the VIRTUAL reflect-padded scene and converts them to
// float32 in the same pass:
//   out[i][c][y][x] = (float) src[c][refl(row_off[i] + y - pad_top, H)][refl(col_off[i] + x - pad_left, W)]   [ * scale ]
//   refl(t, n) = t < 0 ? -t : (t >= n ? 2 (n - 1) - t : t)            (numpy "reflect"; one reflection: pads < n)
// The padded scene is never stored and a uint16 scene stays uint16 in memory; the source is read in place through element strides.
//   Mapping (that of sc_window_cut): the output is a dense stream, cut into 16 KiB pieces of one (window, channel) plane per
//   work-group of 256 threads; a thread owns four 16-byte vectors 4 KiB apart, consecutive lanes hold consecutive vectors of an output
//   row, so one wave-instruction stores 1 KiB contiguously and reads one contiguous run of a source row.  The four source elements of
//   a vector come in one load (8 bytes of uint16, 16 bytes of float32) when they are contiguous (unit column stride), inside the image
//   and aligned to that load; element by element on the reflected fringes, at unaligned columns and at non-unit column strides.
//   Every address is formed in 64 bits.  After the reflection the coordinate is clamped into the image, so whatever the device table
//   holds nothing outside the source is dereferenced; the host copy of the table is what the argument checks read.
// No LDS, no atomics, plain stores inside `out` only: repeated calls give identical bits.
#include <limits.h>

#include "sc_common.h"

namespace {

constexpr int SG_WG = 256;
constexpr int SG_PER_THREAD = 4;
constexpr unsigned SG_CHUNK = SG_WG * SG_PER_THREAD;      // 16-byte output vectors per work-group

struct SceneD {
  const void* src;
  const sc_scene_win* win;
  float* out;
  long long cs, rs, xs;                          // element strides of channel, row, column
  int C, H, W, pad_top, pad_left;
  unsigned vpr, vpp, chunks;                     // vectors per output row / per output plane, work-groups per plane
  float scale;
};

__device__ __forceinline__ long long sg_refl(long long t, long long n) {
  t = t < 0 ? -t : (t >= n ? 2 * (n - 1) - t : t);
  return t < 0 ? 0 : (t >= n ? n - 1 : t);        // (no effect on a checked table)
}

template <class T>
struct alignas(4 * sizeof(T)) SgPack {
  T v[4];
};

// grid.x = n * C * chunks work-groups
template <class T, bool SCALE>
__global__ __launch_bounds__(SG_WG) void k_scene_gather(const SceneD a) {
  const unsigned wc = blockIdx.x / a.chunks, ch = blockIdx.x - wc * a.chunks;
  const unsigned w = wc / (unsigned)a.C, c = wc - w * (unsigned)a.C;
  const long long ro = (long long)a.win[w].row_off - a.pad_top, co = (long long)a.win[w].col_off - a.pad_left;
  const T* s = static_cast<const T*>(a.src) + (long long)c * a.cs;
  float* o = a.out + (size_t)wc * a.vpp * 4;
  const long long H = a.H, W = a.W, xs = a.xs;
#pragma unroll
  for (int k = 0; k < SG_PER_THREAD; ++k) {
    const unsigned t = ch * SG_CHUNK + k * SG_WG + threadIdx.x;
    if (t < a.vpp) {
      const unsigned i = t / a.vpr, jv = t - i * a.vpr;
      const T* row = s + sg_refl(ro + i, H) * a.rs;
      const long long x0 = co + 4ll * jv;
      SgPack<T> r;
      if (xs == 1 && x0 >= 0 && x0 + 4 <= W && (reinterpret_cast<uintptr_t>(row + x0) & (sizeof(r) - 1)) == 0) {
        r = *reinterpret_cast<const SgPack<T>*>(row + x0);
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) r.v[u] = row[sg_refl(x0 + u, W) * xs];
      }
      float4 f = make_float4((float)r.v[0], (float)r.v[1], (float)r.v[2], (float)r.v[3]);
      if (SCALE) { f.x *= a.scale; f.y *= a.scale; f.z *= a.scale; f.w *= a.scale; }
      *reinterpret_cast<float4*>(o + (size_t)t * 4) = f;
    }
  }
}

}  // namespace

extern "C" int sc_scene_gather(const sc_scene_args* a, sc_stream stream) {
  SC_REQUIRE(a, "sc_scene_gather: null arguments");
  SC_REQUIRE(a->src && a->out && a->win && a->win_host, "sc_scene_gather: null pointer");
  SC_REQUIRE(a->elem_bytes == 2 || a->elem_bytes == 4, "sc_scene_gather: element width %d (2 = uint16 or 4 = float32 expected)", a->elem_bytes);
  SC_REQUIRE(a->C >= 1 && a->H >= 1 && a->W >= 1, "sc_scene_gather: bad scene dims %d x %d x %d", a->C, a->H, a->W);
  SC_REQUIRE(a->chan_stride >= 0 && a->row_stride >= 0 && a->col_stride >= 0, "sc_scene_gather: negative stride");
  SC_REQUIRE((uintptr_t)a->src % a->elem_bytes == 0, "sc_scene_gather: the source is not aligned to its %d-byte elements", a->elem_bytes);
  SC_REQUIRE(a->pad_top >= 0 && a->pad_top < a->H && a->pad_left >= 0 && a->pad_left < a->W,
             "sc_scene_gather: reflect padding (%d, %d) needs the image (%d x %d) to be larger than the pad", a->pad_top, a->pad_left, a->H, a->W);
  SC_REQUIRE(a->n >= 1 && a->n <= (1 << 20), "sc_scene_gather: n=%d outside [1, 2^20]", a->n);
  SC_REQUIRE(a->win_h >= 1 && a->win_w >= 4 && a->win_w % 4 == 0 && (long long)a->win_h * a->win_w < (1ll << 31),
             "sc_scene_gather: bad window size %d x %d (the width must be a multiple of 4)", a->win_h, a->win_w);
  SC_REQUIRE((uintptr_t)a->out % 16 == 0 && (uintptr_t)a->win % 4 == 0, "sc_scene_gather: misaligned output or window table");
  SC_REQUIRE(a->scale == a->scale, "sc_scene_gather: scale is NaN");
  for (int i = 0; i < a->n; ++i) {
    const sc_scene_win& q = a->win_host[i];
    // one reflection: rows -pad_top .. 2H - 2 - pad_top of the padded scene exist, i.e. the bottom / right pad is below H / W too
    SC_REQUIRE(q.row_off >= 0 && q.col_off >= 0 && (long long)q.row_off + a->win_h - a->pad_top <= 2ll * a->H - 1 &&
                   (long long)q.col_off + a->win_w - a->pad_left <= 2ll * a->W - 1,
               "sc_scene_gather: window %d (row %d, col %d, %d x %d) leaves the reflect-padded scene (pads must stay below the image size)",
               i, q.row_off, q.col_off, a->win_h, a->win_w);
  }
  SceneD d;
  d.src = a->src; d.win = a->win; d.out = a->out;
  d.cs = a->chan_stride; d.rs = a->row_stride; d.xs = a->col_stride;
  d.C = a->C; d.H = a->H; d.W = a->W; d.pad_top = a->pad_top; d.pad_left = a->pad_left;
  d.vpr = (unsigned)(a->win_w / 4);
  d.vpp = d.vpr * (unsigned)a->win_h;
  d.chunks = (d.vpp + SG_CHUNK - 1) / SG_CHUNK;
  d.scale = a->scale;
  const long long blocks = (long long)a->n * a->C * d.chunks;
  SC_REQUIRE(blocks <= INT_MAX, "sc_scene_gather: grid of %lld work-groups is too large for one launch", blocks);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)blocks), wg(SG_WG);
  const bool sc = a->scale != 1.0f;
  if (a->elem_bytes == 2) {
    if (sc) hipLaunchKernelGGL((k_scene_gather<uint16_t, true>), grid, wg, 0, st, d);
    else hipLaunchKernelGGL((k_scene_gather<uint16_t, false>), grid, wg, 0, st, d);
  } else {
    if (sc) hipLaunchKernelGGL((k_scene_gather<float, true>), grid, wg, 0, st, d);
    else hipLaunchKernelGGL((k_scene_gather<float, false>), grid, wg, 0, st, d);
  }
  SC_LAUNCH_OK("sc_scene_gather");
  return SC_OK;
}
