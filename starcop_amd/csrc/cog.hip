// Cloud-Optimized GeoTIFF products on the device (starcop_amd/cog.py: write_cog; the reference writes every product with
// georeader.save_cog): what touches every pixel of a product -- the overview pyramid, the cut into TIFF tiles with their zero
// padding and predictor, and the search for tiles that hold nothing but fill -- runs here; only the tiles that will be stored
// cross to the host, which deflates them.
//   sc_overview_reduce : one launch halves an image up to three times.  A work-group of 256 threads owns an aligned 64 x 64
//     block of one band of the source, reads it once (16-byte loads where the column stride is 1, the run lies inside the image
//     and its address is 16-byte aligned; element loads otherwise), keeps the 32 x 32, 16 x 16 and 8 x 8 results in LDS and
//     writes all three (16-byte stores where the destination width keeps the rows aligned).  Level k + 1 is computed from the
//     STORED bits of level k with the same one-level operator, so one launch of three levels and three launches of one level
//     give identical bytes.  The float average sums in float64 in the fixed order (0,0), (0,1), (1,0), (1,1), every operation
//     rounded on its own (contraction off).
//   sc_tiff_tile_flags : one work-group per tile: flags[tile] = every in-image sample has the bits of the fill value.
//   sc_tiff_pack_tiles : one work-group per (stored tile, chunk of tile rows): the rows are staged into LDS pixel-interleaved
//     (band-planar 16-byte loads in, zero beyond the image edge), then written as finished TIFF bytes in 16-byte stores with
//     predictor 1 (none), 2 (uint8: horizontal difference) or 3 (float32: bytes by significance, then difference).
// Integer LDS atomics only (the flag of a tile); no floating-point atomics, no work-group waits on another: two calls give
// identical bytes.
#include <limits.h>
#include <string.h>

#include <vector>

#include "sc_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int COG_WG = 256;
constexpr int COG_PACK_LDS = 32768;              // bytes of tile rows a pack work-group stages at a time
constexpr unsigned COG_NAN = 0x7FC00000u;        // numpy's float32 NaN

struct ImgD {
  const void* p;
  long long bstride, rs, cs;                     // elements
  int nb, h, w, has_nd;
  unsigned nd;
};

template <class T, int V>
struct alignas(16) CPack {
  T v[V];
};

// V = 16 / sizeof(T) consecutive elements of row r of one band from column c on; zero where the image ends
template <class T>
__device__ __forceinline__ void load_run(const T* band, long long rs, long long cs, int h, int w, long long r, long long c,
                                         CPack<T, 16 / (int)sizeof(T)>& o) {
  constexpr int V = 16 / (int)sizeof(T);
  if (r < h && c + V <= w) {
    const T* q = band + r * rs + c * cs;
    if (cs == 1) {
      if ((reinterpret_cast<uintptr_t>(q) & 15) == 0) o = *reinterpret_cast<const CPack<T, V>*>(q);
      else __builtin_memcpy(&o, q, sizeof(o));
    } else {
#pragma unroll
      for (int u = 0; u < V; ++u) o.v[u] = q[u * cs];
    }
  } else {
#pragma unroll
    for (int u = 0; u < V; ++u) o.v[u] = (r < h && c + u < w) ? band[r * rs + (c + u) * cs] : (T)0;
  }
}

__device__ __forceinline__ bool cog_valid(uint32_t v, bool has_nd, uint32_t nd) {
  return (v & 0x7FFFFFFFu) <= 0x7F800000u && !(has_nd && v == nd);        // not NaN, not the nodata bits (-0.0 is not 0.0)
}
__device__ __forceinline__ bool cog_valid(uint8_t v, bool has_nd, uint8_t nd) { return !(has_nd && v == nd); }

// the one-level operator on the 2 x 2 source samples (0,0), (0,1), (1,0), (1,1); in[k]: sample k lies inside the image
template <class T>
__device__ __forceinline__ T reduce4(const T (&v)[4], const bool (&in)[4], int mode, bool has_nd, T nd) {
  if (mode == SC_COG_NEAREST) return v[0];
  bool ok[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) ok[k] = in[k] && cog_valid(v[k], has_nd, nd);
  if constexpr (sizeof(T) == 4) {
    double s = 0.0;
    int n = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (ok[k]) {
        const double x = (double)__uint_as_float(v[k]);
        s = n ? s + x : x;
        ++n;
      }
    if (n == 0) return has_nd ? nd : (T)COG_NAN;
    return (T)__float_as_uint((float)(s / (double)n));
  } else {
    if (mode == SC_COG_AVERAGE) {
      unsigned s = 0, n = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (ok[k]) { s += v[k]; ++n; }
      return n ? (T)((2u * s + n) / (2u * n)) : (has_nd ? nd : (T)0);
    }
    int best_n = 0;
    unsigned best_v = has_nd ? nd : 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (!ok[k]) continue;
      int n = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) n += (ok[j] && v[j] == v[k]) ? 1 : 0;
      if (n > best_n || (n == best_n && v[k] < best_v)) { best_n = n; best_v = v[k]; }
    }
    return (T)best_v;
  }
}

struct OvD {
  ImgD s;
  int mode, levels;
  void* dst[3];
  int dh[3], dw[3];
};

// the N x N block of a level, held in LDS, to rows R0.., columns C0.. of band b of its dense (nb, dh, dw) destination
template <class T, int N>
__device__ __forceinline__ void store_block(const T* l, void* dst, int dh, int dw, int b, long long R0, long long C0) {
  constexpr int V = 16 / (int)sizeof(T);
  T* o = static_cast<T*>(dst) + (size_t)b * dh * dw;
  if constexpr (N % V == 0) {
    if (dw % V == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {          // every row of every band starts 16-byte aligned
      for (int it = threadIdx.x; it < N * (N / V); it += COG_WG) {
        const int i = it / (N / V), j = it - i * (N / V);
        const long long r = R0 + i, c = C0 + (long long)j * V;
        if (r < dh && c < dw) *reinterpret_cast<CPack<T, V>*>(o + r * dw + c) = *reinterpret_cast<const CPack<T, V>*>(l + i * N + j * V);
      }
      return;
    }
  }
  for (int it = threadIdx.x; it < N * N; it += COG_WG) {
    const int i = it / N, j = it - i * N;
    const long long r = R0 + i, c = C0 + j;
    if (r < dh && c < dw) o[r * dw + c] = l[it];
  }
}

// level k + 1 (M x M, M = N / 2) of a block from the N x N level k in LDS; (R0, C0): origin of the block in level k
template <class T, int N>
__device__ __forceinline__ void next_level(const T* l, T* o, int ph, int pw, long long R0, long long C0, int mode, bool has_nd, T nd) {
  constexpr int M = N / 2;
  for (int t = threadIdx.x; t < M * M; t += COG_WG) {
    const int i = t / M, j = t - i * M;
    const long long r = R0 + 2 * i, c = C0 + 2 * j;
    const T v[4] = {l[(2 * i) * N + 2 * j], l[(2 * i) * N + 2 * j + 1], l[(2 * i + 1) * N + 2 * j], l[(2 * i + 1) * N + 2 * j + 1]};
    const bool in[4] = {r < ph && c < pw, r < ph && c + 1 < pw, r + 1 < ph && c < pw, r + 1 < ph && c + 1 < pw};
    o[t] = in[0] ? reduce4<T>(v, in, mode, has_nd, nd) : (T)0;
  }
}

// grid = (ceil(w / 64), ceil(h / 64), nb)
template <class T>
__global__ __launch_bounds__(COG_WG) void k_overview(OvD a) {
  constexpr int V = 16 / (int)sizeof(T), VPR = 64 / V, H2 = V / 2;
  __shared__ __attribute__((aligned(16))) T l1[32 * 32];
  __shared__ __attribute__((aligned(16))) T l2[16 * 16];
  __shared__ __attribute__((aligned(16))) T l3[8 * 8];
  const int b = blockIdx.z, h = a.s.h, w = a.s.w, mode = a.mode;
  const long long r0 = (long long)blockIdx.y * 64, c0 = (long long)blockIdx.x * 64;
  const T* band = static_cast<const T*>(a.s.p) + (long long)b * a.s.bstride;
  const bool has_nd = a.s.has_nd != 0;
  const T nd = (T)a.s.nd;
  for (int it = threadIdx.x; it < 32 * VPR; it += COG_WG) {
    const int rp = it / VPR, vx = it - rp * VPR;
    const long long r = r0 + 2 * rp, c = c0 + vx * V;
    CPack<T, V> top, bot;
    load_run<T>(band, a.s.rs, a.s.cs, h, w, r, c, top);
    load_run<T>(band, a.s.rs, a.s.cs, h, w, r + 1, c, bot);
#pragma unroll
    for (int k = 0; k < H2; ++k) {
      const long long cc = c + 2 * k;
      const T v[4] = {top.v[2 * k], top.v[2 * k + 1], bot.v[2 * k], bot.v[2 * k + 1]};
      const bool in[4] = {r < h && cc < w, r < h && cc + 1 < w, r + 1 < h && cc < w, r + 1 < h && cc + 1 < w};
      l1[rp * 32 + vx * H2 + k] = in[0] ? reduce4<T>(v, in, mode, has_nd, nd) : (T)0;
    }
  }
  __syncthreads();
  store_block<T, 32>(l1, a.dst[0], a.dh[0], a.dw[0], b, r0 / 2, c0 / 2);
  if (a.levels < 2) return;
  next_level<T, 32>(l1, l2, a.dh[0], a.dw[0], r0 / 2, c0 / 2, mode, has_nd, nd);
  __syncthreads();
  store_block<T, 16>(l2, a.dst[1], a.dh[1], a.dw[1], b, r0 / 4, c0 / 4);
  if (a.levels < 3) return;
  next_level<T, 16>(l2, l3, a.dh[1], a.dw[1], r0 / 4, c0 / 4, mode, has_nd, nd);
  __syncthreads();
  store_block<T, 8>(l3, a.dst[2], a.dh[2], a.dw[2], b, r0 / 8, c0 / 8);
}

// grid = tiles (row-major); flags[tile] = 1 where every in-image sample of the tile has the bits of `fill`
template <class T>
__global__ __launch_bounds__(COG_WG) void k_tile_flags(ImgD s, int bs, int tx, unsigned fill32, uint8_t* flags) {
  constexpr int V = 16 / (int)sizeof(T);
  __shared__ int differs;
  if (threadIdx.x == 0) differs = 0;
  __syncthreads();
  const int ty = blockIdx.x / tx, txi = blockIdx.x - ty * tx;
  const long long r0 = (long long)ty * bs, c0 = (long long)txi * bs;
  const int nr = (int)(s.h - r0 < bs ? s.h - r0 : bs), ncol = (int)(s.w - c0 < bs ? s.w - c0 : bs);
  const int vpr = (ncol + V - 1) / V, per_band = nr * vpr;
  const T fill = (T)fill32;
  bool d = false;
  for (int it = threadIdx.x; it < s.nb * per_band; it += COG_WG) {
    const int b = it / per_band, rem = it - b * per_band, i = rem / vpr, jv = rem - i * vpr;
    const long long c = c0 + (long long)jv * V;
    CPack<T, V> v;
    load_run<T>(static_cast<const T*>(s.p) + (long long)b * s.bstride, s.rs, s.cs, s.h, s.w, r0 + i, c, v);
#pragma unroll
    for (int u = 0; u < V; ++u) d |= (c + u < s.w) && v.v[u] != fill;
  }
  if (d) atomicOr(&differs, 1);
  __syncthreads();
  if (threadIdx.x == 0) flags[blockIdx.x] = differs ? 0 : 1;
}

struct PackD {
  ImgD s;
  int bs, predictor, tx, R, chunks;              // R tile rows per work-group, chunks = ceil(bs / R) work-groups per tile
  const int32_t* slots;
  uint8_t* out;
};

// byte i of a predictor-3 row before differencing: byte (3 - plane) of sample (i - plane * n), n samples per row
__device__ __forceinline__ unsigned fp_byte(const uint8_t* lr, int i, int n) {
  const int plane = i / n, sidx = i - plane * n;
  return lr[sidx * 4 + 3 - plane];
}

// grid = tiles * chunks; dynamic LDS: R * bs * nb * sizeof(T) bytes
template <class T>
__global__ __launch_bounds__(COG_WG) void k_pack_tiles(PackD a) {
  constexpr int V = 16 / (int)sizeof(T);
  extern __shared__ __attribute__((aligned(16))) uint8_t cog_smem[];
  T* lds = reinterpret_cast<T*>(cog_smem);
  const unsigned tile = blockIdx.x / (unsigned)a.chunks, ch = blockIdx.x - tile * (unsigned)a.chunks;
  const int slot = a.slots[tile];
  if (slot < 0) return;
  const int bs = a.bs, nb = a.s.nb;
  const int ty = (int)(tile / (unsigned)a.tx), txi = (int)(tile - (unsigned)ty * (unsigned)a.tx);
  const int i0 = (int)ch * a.R, nr = bs - i0 < a.R ? bs - i0 : a.R;
  const int vpr = bs / V, per_band = nr * vpr;
  const long long r0 = (long long)ty * bs + i0, c0 = (long long)txi * bs;
  for (int it = threadIdx.x; it < nb * per_band; it += COG_WG) {
    const int b = it / per_band, rem = it - b * per_band, i = rem / vpr, jv = rem - i * vpr;
    CPack<T, V> v;
    load_run<T>(static_cast<const T*>(a.s.p) + (long long)b * a.s.bstride, a.s.rs, a.s.cs, a.s.h, a.s.w, r0 + i, c0 + (long long)jv * V, v);
    T* q = lds + ((size_t)i * bs + (size_t)jv * V) * nb + b;
#pragma unroll
    for (int u = 0; u < V; ++u) q[u * nb] = v.v[u];
  }
  __syncthreads();
  const int n = bs * nb, row_bytes = n * (int)sizeof(T), vrow = row_bytes / 16;
  uint8_t* o = a.out + (size_t)slot * bs * row_bytes + (size_t)i0 * row_bytes;
  for (int it = threadIdx.x; it < nr * vrow; it += COG_WG) {
    const int row = it / vrow, k0 = (it - row * vrow) * 16;
    const uint8_t* lr = cog_smem + (size_t)row * row_bytes;
    CPack<uint8_t, 16> r;
    if (a.predictor == 1) {
      r = *reinterpret_cast<const CPack<uint8_t, 16>*>(lr + k0);
    } else if (a.predictor == 2) {
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int k = k0 + u;
        r.v[u] = (uint8_t)(lr[k] - (k >= nb ? lr[k - nb] : 0));
      }
    } else {
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int i = k0 + u;
        r.v[u] = (uint8_t)(fp_byte(lr, i, n) - (i >= nb ? fp_byte(lr, i - nb, n) : 0u));
      }
    }
    *reinterpret_cast<CPack<uint8_t, 16>*>(o + (size_t)row * row_bytes + k0) = r;
  }
}

int check_image(const sc_cog_image* s, const char* who, ImgD* d) {
  SC_REQUIRE(s->data, "%s: null source", who);
  SC_REQUIRE(s->elem_bytes == 1 || s->elem_bytes == 4, "%s: element width %d (1 = uint8 or 4 = float32 expected)", who, s->elem_bytes);
  SC_REQUIRE(s->nb >= 1 && s->nb <= SC_COG_MAX_BANDS, "%s: nb=%d outside [1, %d]", who, s->nb, SC_COG_MAX_BANDS);
  SC_REQUIRE(s->h >= 1 && s->w >= 1, "%s: bad image size %d x %d", who, s->h, s->w);
  SC_REQUIRE(s->band_stride >= 0 && s->row_stride >= 0 && s->col_stride >= 0, "%s: negative stride", who);
  SC_REQUIRE((uintptr_t)s->data % s->elem_bytes == 0, "%s: the source is not aligned to its %d-byte elements", who, s->elem_bytes);
  SC_REQUIRE(s->has_nodata == 0 || s->has_nodata == 1, "%s: has_nodata=%d", who, s->has_nodata);
  if (s->has_nodata && s->elem_bytes == 1) SC_REQUIRE((s->nodata_bits >> 8) == 0, "%s: nodata pattern 0x%x is wider than a byte", who, s->nodata_bits);
  d->p = s->data; d->bstride = s->band_stride; d->rs = s->row_stride; d->cs = s->col_stride;
  d->nb = s->nb; d->h = s->h; d->w = s->w; d->has_nd = s->has_nodata; d->nd = s->has_nodata ? s->nodata_bits : 0u;
  return SC_OK;
}

}  // namespace

extern "C" int sc_overview_reduce(const sc_overview_args* a, sc_stream stream) {
  SC_REQUIRE(a, "sc_overview_reduce: null arguments");
  OvD d;
  if (int rc = check_image(&a->src, "sc_overview_reduce", &d.s)) return rc;
  const int eb = a->src.elem_bytes;
  SC_REQUIRE(a->resampling == SC_COG_AVERAGE || a->resampling == SC_COG_NEAREST || a->resampling == SC_COG_MODE,
             "sc_overview_reduce: unknown resampling %d", a->resampling);
  SC_REQUIRE(!(a->resampling == SC_COG_MODE && eb != 1), "sc_overview_reduce: mode resampling is for uint8 images");
  SC_REQUIRE(a->levels >= 1 && a->levels <= 3, "sc_overview_reduce: levels=%d outside [1, 3]", a->levels);
  int h = a->src.h, w = a->src.w;
  for (int k = 0; k < 3; ++k) {
    h = (h + 1) / 2; w = (w + 1) / 2;
    const bool on = k < a->levels;
    if (on) SC_REQUIRE(a->dst[k] && (uintptr_t)a->dst[k] % eb == 0, "sc_overview_reduce: null or misaligned destination %d", k);
    d.dst[k] = on ? a->dst[k] : nullptr; d.dh[k] = h; d.dw[k] = w;
  }
  const long long gy = ((long long)a->src.h + 63) / 64, gx = ((long long)a->src.w + 63) / 64;
  SC_REQUIRE(gy <= 65535, "sc_overview_reduce: %d rows are too many for one launch (64 x 65535 at most)", a->src.h);
  d.mode = a->resampling; d.levels = a->levels;
  const dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)a->src.nb);
  hipStream_t st = (hipStream_t)stream;
  if (eb == 4) hipLaunchKernelGGL((k_overview<uint32_t>), grid, dim3(COG_WG), 0, st, d);
  else hipLaunchKernelGGL((k_overview<uint8_t>), grid, dim3(COG_WG), 0, st, d);
  SC_LAUNCH_OK("sc_overview_reduce");
  return SC_OK;
}

static int tile_grid(const sc_cog_image* s, int bs, const char* who, int* ty, int* tx) {
  SC_REQUIRE(bs >= 16 && bs % 16 == 0, "%s: tile size %d is not a positive multiple of 16", who, bs);
  SC_REQUIRE((long long)bs * s->nb * s->elem_bytes <= COG_PACK_LDS, "%s: a tile row of %d pixels x %d bands x %d bytes exceeds %d bytes", who, bs,
             s->nb, s->elem_bytes, COG_PACK_LDS);
  const long long y = ((long long)s->h + bs - 1) / bs, x = ((long long)s->w + bs - 1) / bs;
  SC_REQUIRE(y * x <= (1 << 24), "%s: %lld tiles are too many for one launch (2^24 at most)", who, y * x);
  *ty = (int)y; *tx = (int)x;
  return SC_OK;
}

extern "C" int sc_tiff_tile_flags(const sc_cog_image* src, int bs, uint8_t* flags, sc_stream stream) {
  SC_REQUIRE(src && flags, "sc_tiff_tile_flags: null pointer");
  ImgD d;
  if (int rc = check_image(src, "sc_tiff_tile_flags", &d)) return rc;
  int ty, tx;
  if (int rc = tile_grid(src, bs, "sc_tiff_tile_flags", &ty, &tx)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (src->elem_bytes == 4) hipLaunchKernelGGL((k_tile_flags<uint32_t>), dim3((unsigned)(ty * tx)), dim3(COG_WG), 0, st, d, bs, tx, d.nd, flags);
  else hipLaunchKernelGGL((k_tile_flags<uint8_t>), dim3((unsigned)(ty * tx)), dim3(COG_WG), 0, st, d, bs, tx, d.nd, flags);
  SC_LAUNCH_OK("sc_tiff_tile_flags");
  return SC_OK;
}

extern "C" int sc_tiff_pack_tiles(const sc_tiff_pack_args* a, sc_stream stream) {
  SC_REQUIRE(a, "sc_tiff_pack_tiles: null arguments");
  PackD d;
  if (int rc = check_image(&a->src, "sc_tiff_pack_tiles", &d.s)) return rc;
  int ty, tx;
  if (int rc = tile_grid(&a->src, a->bs, "sc_tiff_pack_tiles", &ty, &tx)) return rc;
  const int eb = a->src.elem_bytes, tiles = ty * tx;
  SC_REQUIRE(a->predictor == 1 || (a->predictor == 2 && eb == 1) || (a->predictor == 3 && eb == 4),
             "sc_tiff_pack_tiles: predictor %d on %d-byte samples (1; 2 on uint8; 3 on float32)", a->predictor, eb);
  SC_REQUIRE(a->slots && a->slots_host, "sc_tiff_pack_tiles: null slot table");
  SC_REQUIRE((uintptr_t)a->slots % 4 == 0, "sc_tiff_pack_tiles: misaligned slot table");
  SC_REQUIRE(a->n_slots >= 0, "sc_tiff_pack_tiles: n_slots=%d", a->n_slots);
  const size_t tile_bytes = (size_t)a->bs * a->bs * a->src.nb * eb;
  SC_REQUIRE(a->out_bytes >= (size_t)a->n_slots * tile_bytes, "sc_tiff_pack_tiles: the output holds %zu bytes, %d tiles of %zu need more",
             a->out_bytes, a->n_slots, tile_bytes);
  {
    std::vector<uint8_t> seen((size_t)a->n_slots, 0);
    for (int t = 0; t < tiles; ++t) {
      const int32_t s = a->slots_host[t];
      if (s == -1) continue;
      SC_REQUIRE(s >= 0 && s < a->n_slots, "sc_tiff_pack_tiles: slot %d of tile %d outside [0, %d)", s, t, a->n_slots);
      SC_REQUIRE(!seen[(size_t)s], "sc_tiff_pack_tiles: slot %d is given to two tiles", s);
      seen[(size_t)s] = 1;
    }
  }
  if (a->n_slots == 0) return SC_OK;
  SC_REQUIRE(a->out && (uintptr_t)a->out % 16 == 0, "sc_tiff_pack_tiles: null or misaligned output");
  hipStream_t st = (hipStream_t)stream;
  {
    // the device copy of the table is what the kernel walks: it must be the table that was just checked
    std::vector<int32_t> dev((size_t)tiles);
    const size_t bytes = dev.size() * sizeof(int32_t);
    if (hipMemcpyAsync(dev.data(), a->slots, bytes, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
      (void)hipGetLastError();
      sc_set_error("sc_tiff_pack_tiles: reading back the device slot table failed");
      return SC_ERR_LAUNCH;
    }
    SC_REQUIRE(memcmp(dev.data(), a->slots_host, bytes) == 0, "sc_tiff_pack_tiles: the host and device slot tables differ");
  }
  const int row_bytes = a->bs * a->src.nb * eb;
  d.bs = a->bs; d.predictor = a->predictor; d.tx = tx;
  d.R = COG_PACK_LDS / row_bytes < a->bs ? COG_PACK_LDS / row_bytes : a->bs;
  d.chunks = (a->bs + d.R - 1) / d.R;
  d.slots = a->slots; d.out = static_cast<uint8_t*>(a->out);
  const long long blocks = (long long)tiles * d.chunks;
  SC_REQUIRE(blocks <= INT_MAX, "sc_tiff_pack_tiles: grid of %lld work-groups is too large for one launch", blocks);
  const size_t lds = (size_t)d.R * row_bytes;
  if (eb == 4) hipLaunchKernelGGL((k_pack_tiles<uint32_t>), dim3((unsigned)blocks), dim3(COG_WG), lds, st, d);
  else hipLaunchKernelGGL((k_pack_tiles<uint8_t>), dim3((unsigned)blocks), dim3(COG_WG), lds, st, d);
  SC_LAUNCH_OK("sc_tiff_pack_tiles");
  return SC_OK;
}
