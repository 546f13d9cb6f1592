// Mosaic: N rasters on grids of their own composed into one raster on a destination grid in ONE launch (sc_mosaic, starcop_hip.h).
//   The projection, the extent test and the sampling are those of the warp (sc_warp.h): a mosaic of one source is the warp of it.
//   What one kernel buys over N warps and a chain of selects:
//   - the Krueger INVERSE series of a destination pixel (UTM destination) is summed once, not once per source; the FORWARD series of
//     sources in another zone once per run of sources that share the zone; sources in the destination's CRS or in 4326 cost an affine;
//   - a work-group tests its tile against the destination-pixel box of every source (uniform: the descriptors come through scalar
//     loads) and runs the per-source work only for the boxes it meets; a tile that meets none writes no-data and returns before any
//     projection;
//   - no full-grid intermediates: the winner rules keep (index, u, v) of the best source in registers -- the key plane's nearest
//     element is the only memory read of that pass -- and sample the P planes of the winner afterwards (lanes read their winner's
//     descriptor themselves: a lane's row of the table, a few hundred bytes that stay in the vector cache); `mean` keeps an fp64 sum
//     and a term count per plane (at most SC_MOSAIC_MEAN_PLANES planes per launch).
//   The source loop is a runtime loop over the set bits of the tile's source mask and is NOT unrolled: every copy would repeat the
//   ~20 fp64 transcendental call sites of the forward series.  Mapping as k_warp: 256 threads own 16 rows x 64 pixels, a thread 4
//   consecutive pixels (2 for 8-byte elements) and one 16-byte store per plane; one pixel per thread and 4 rows x 64 pixels when the
//   width is not a multiple of the vector or an output is not aligned to the store.  No LDS, no atomics: two calls give the same bytes.
#include <limits.h>

#include <cmath>

#include "sc_common.h"
#include "sc_warp.h"

namespace {

constexpr int MOS_PMAX = SC_WARP_MAX_PLANES;
constexpr int MOS_MEANP = SC_MOSAIC_MEAN_PLANES;
constexpr int MOS_WG = 256;

struct MosD {
  double gt[6];
  Krueger k;
  double dst_lon0, dst_fn;                       // central meridian (degrees) and false northing of a UTM destination
  int dst_kind;                                  // 1 geographic, 2 UTM; 0: every source carries the destination's code (affine only)
  int dst_crs;
  int H, W, P, N, tiles_x;
  int rule, key, keyfloat;
  const sc_mosaic_source* tab;
  void* out;
  int* index;
  int* count;
  const int* select;
  unsigned long long nod[MOS_PMAX];
};

template <class T>
__device__ __forceinline__ bool is_nan_bits(T b) {
  if constexpr (sizeof(T) == 4) return (b & 0x7FFFFFFFu) > 0x7F800000u;
  else if constexpr (sizeof(T) == 8) return (b & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull;
  else return false;
}

// grid.x = tiles_y * tiles_x tiles of TY rows x TX * V pixels.  BIL: bilinear; MEAN: the mean rule (both: T = uint32_t, float32 bits)
template <class T, int V, bool BIL, bool MEAN>
__global__ __launch_bounds__(MOS_WG) void k_mosaic(MosD a) {
  constexpr int TX = V == 1 ? 64 : 16, TY = MOS_WG / TX;
  constexpr int NP = MEAN ? MOS_MEANP : 1;
  const sc_mosaic_source* __restrict__ tab = a.tab;
  const int by = blockIdx.x / a.tiles_x, bx = blockIdx.x - by * a.tiles_x;
  const int tr0 = by * TY, tr1 = tr0 + TY;
  const long long tc0 = (long long)bx * (TX * V), tc1 = tc0 + TX * V;
  // the sources whose box meets this tile, and whether one of them needs longitude / latitude: the same in every lane
  unsigned long long live = 0;
  bool need_ll = false;
  for (int s = 0; s < a.N; ++s) {
    const sc_mosaic_source& d = tab[s];
    if (d.box[0] < tr1 && d.box[1] > tr0 && d.box[2] < tc1 && d.box[3] > tc0) {
      live |= 1ull << s;
      need_ll = need_ll || d.src_crs != a.dst_crs;
    }
  }
  const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;
  const long long x0 = tc0 + (long long)tx * V;
  const int y = tr0 + ty;
  if (y >= a.H || x0 >= a.W) return;              // W % V == 0 on the vector path: a thread's V pixels are inside the row or all outside
  const size_t pix = (size_t)y * a.W + (size_t)x0;
  const size_t plane = (size_t)a.H * a.W;
  T* o = static_cast<T*>(a.out) + pix;
  if (live == 0) {                                // no source has a pixel here: nothing is projected
    for (int p = 0; p < a.P; ++p) {
      Pack<T, V> r;
#pragma unroll
      for (int e = 0; e < V; ++e) r.v[e] = (T)a.nod[p];
      *reinterpret_cast<Pack<T, V>*>(o + (size_t)p * plane) = r;
    }
    Pack<int, V> none, zero;
#pragma unroll
    for (int e = 0; e < V; ++e) { none.v[e] = -1; zero.v[e] = 0; }
    if (a.index) *reinterpret_cast<Pack<int, V>*>(a.index + pix) = none;
    if (a.count) *reinterpret_cast<Pack<int, V>*>(a.count + pix) = zero;
    return;
  }
  double wx[V], wy[V], lon[V], lat[V];            // world coordinates in the destination's CRS; longitude / latitude
  bool llok[V];
#pragma unroll
  for (int e = 0; e < V; ++e) {
    const double px = (double)(x0 + e) + 0.5, py = (double)y + 0.5;
    wx[e] = a.gt[0] + px * a.gt[1] + py * a.gt[2];
    wy[e] = a.gt[3] + px * a.gt[4] + py * a.gt[5];
    lon[e] = wx[e]; lat[e] = wy[e]; llok[e] = true;
  }
  if (a.dst_kind == 2 && need_ll) {
#pragma unroll
    for (int e = 0; e < V; ++e) llok[e] = tm_inverse(a.k, a.dst_lon0, a.dst_fn, wx[e], wy[e], lon[e], lat[e]);
  }
  double fe[V], fn[V];                            // easting / northing in the zone `fwd_crs`
  bool fok[V];
  int fwd_crs = -1;
  int cnt[V], best[V], sel[V];
  double bu[V], bv[V];
  float bk[V];
  double sum[V][NP];
  int terms[V][NP];
#pragma unroll
  for (int e = 0; e < V; ++e) {
    fe[e] = fn[e] = 0.0; fok[e] = false;
    cnt[e] = 0; best[e] = -1; bu[e] = bv[e] = 0.0; bk[e] = 0.f;
    sel[e] = (!MEAN && a.rule == SC_MOSAIC_BY_INDEX) ? a.select[pix + e] : -1;
#pragma unroll
    for (int p = 0; p < NP; ++p) { sum[e][p] = 0.0; terms[e][p] = 0; }
  }
  const int kidx = a.key > 0 ? a.key : 0;
  const T knod = (T)a.nod[kidx];
  for (unsigned long long m = live; m; m &= m - 1) {      // ascending source numbers; uniform
    const int s = __builtin_ctzll(m);
    const sc_mosaic_source& d = tab[s];
    const int scrs = d.src_crs;
    const bool same = scrs == a.dst_crs, geo = scrs == 4326;
    if (!same && !geo && scrs != fwd_crs) {       // another zone than the previous projected source: the forward series
      const double lon0 = 6.0 * (double)(scrs % 100) - 183.0, fn0 = scrs >= 32701 ? 10000000.0 : 0.0;
#pragma unroll
      for (int e = 0; e < V; ++e) {
        fe[e] = fn[e] = 0.0;
        fok[e] = tm_forward(a.k, lon0, fn0, lon[e], lat[e], fe[e], fn[e]);
      }
      fwd_crs = scrs;
    }
    const double i0 = d.src_inv[0], i1 = d.src_inv[1], i2 = d.src_inv[2], i3 = d.src_inv[3], i4 = d.src_inv[4], i5 = d.src_inv[5];
    const int sh = d.src_h, sw = d.src_w;
    const T* kp = static_cast<const T*>(d.src[kidx]);
    const long long krs = d.row_stride[kidx], kcs = d.col_stride[kidx];
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const double X = same ? wx[e] : (geo ? lon[e] : fe[e]);
      const double Y = same ? wy[e] : (geo ? lat[e] : fn[e]);
      const bool ok = same || (llok[e] && (geo || fok[e]));
      const double u = i0 + X * i1 + Y * i2;
      const double v = i3 + X * i4 + Y * i5;
      const bool inside = ok && u >= 0.0 && u < (double)sw && v >= 0.0 && v < (double)sh;      // false for NaN and infinities
      bool valid = inside;
      T kb = 0;
      if (inside && a.key >= 0) {
        kb = kp[(long long)floor(v) * krs + (long long)floor(u) * kcs];
        valid = kb != knod && !(a.keyfloat && is_nan_bits(kb));
      }
      cnt[e] += valid ? 1 : 0;
      if constexpr (MEAN) {
        if (valid) {
#pragma unroll
          for (int p = 0; p < NP; ++p) {
            if (p < a.P) {
              const uint32_t* sp = static_cast<const uint32_t*>(d.src[p]);
              const long long rs = d.row_stride[p], cs = d.col_stride[p];
              const uint32_t nod = (uint32_t)a.nod[p];
              const uint32_t b = sp[(long long)floor(v) * rs + (long long)floor(u) * cs];
              if (counts(b, nod)) {
                sum[e][p] += BIL ? bilinear_f64(sp, rs, cs, nod, sh, sw, u, v) : (double)__uint_as_float(b);
                terms[e][p] += 1;
              }
            }
          }
        }
      } else {
        bool take;
        float kf = 0.f;
        if constexpr (sizeof(T) == 4) kf = __uint_as_float(kb);
        if (a.rule == SC_MOSAIC_FIRST) take = valid && best[e] < 0;
        else if (a.rule == SC_MOSAIC_LAST) take = valid;
        else if (a.rule == SC_MOSAIC_MAX) take = valid && (best[e] < 0 || kf > bk[e]);
        else if (a.rule == SC_MOSAIC_MIN) take = valid && (best[e] < 0 || kf < bk[e]);
        else take = inside && s == sel[e];
        if (take) { best[e] = s; bu[e] = u; bv[e] = v; bk[e] = kf; }
      }
    }
  }
  if constexpr (MEAN) {
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      if (p < a.P) {
        Pack<T, V> r;
#pragma unroll
        for (int e = 0; e < V; ++e)
          r.v[e] = terms[e][p] ? __float_as_uint((float)(sum[e][p] / (double)terms[e][p])) : (T)a.nod[p];
        *reinterpret_cast<Pack<T, V>*>(o + (size_t)p * plane) = r;
      }
    }
  } else {
    for (int p = 0; p < a.P; ++p) {               // p is uniform; the winner's descriptor is read by the lane
      const T nod = (T)a.nod[p];
      Pack<T, V> r;
#pragma unroll
      for (int e = 0; e < V; ++e) {
        T val = nod;
        if (best[e] >= 0) {
          const sc_mosaic_source& w = tab[best[e]];
          val = sample<T, BIL>(static_cast<const T*>(w.src[p]), w.row_stride[p], w.col_stride[p], nod, w.src_h, w.src_w, bu[e], bv[e], true);
        }
        r.v[e] = val;
      }
      *reinterpret_cast<Pack<T, V>*>(o + (size_t)p * plane) = r;
    }
    if (a.index) {
      Pack<int, V> r;
#pragma unroll
      for (int e = 0; e < V; ++e) r.v[e] = best[e];
      *reinterpret_cast<Pack<int, V>*>(a.index + pix) = r;
    }
  }
  if (a.count) {
    Pack<int, V> r;
#pragma unroll
    for (int e = 0; e < V; ++e) r.v[e] = cnt[e];
    *reinterpret_cast<Pack<int, V>*>(a.count + pix) = r;
  }
}

template <class T, int V, bool BIL, bool MEAN>
int launch(const MosD& d0, bool vec, hipStream_t st) {
  MosD d = d0;
  const int tw = vec ? 16 * V : 64, th = vec ? MOS_WG / 16 : MOS_WG / 64;
  d.tiles_x = (d.W + tw - 1) / tw;
  const long long tiles = (long long)d.tiles_x * ((d.H + th - 1) / th);
  SC_REQUIRE(tiles <= INT_MAX, "sc_mosaic: grid too large for one launch");
  if (vec) hipLaunchKernelGGL((k_mosaic<T, V, BIL, MEAN>), dim3((unsigned)tiles), dim3(MOS_WG), 0, st, d);
  else hipLaunchKernelGGL((k_mosaic<T, 1, BIL, MEAN>), dim3((unsigned)tiles), dim3(MOS_WG), 0, st, d);
  return SC_OK;
}

}  // namespace

extern "C" int sc_mosaic(const sc_mosaic_args* a, sc_stream stream) {
  SC_REQUIRE(a, "sc_mosaic: null arguments");
  SC_REQUIRE(a->N >= 1 && a->N <= SC_MOSAIC_MAX_SOURCES, "sc_mosaic: N=%d sources outside [1, %d]", a->N, SC_MOSAIC_MAX_SOURCES);
  SC_REQUIRE(a->P >= 1 && a->P <= MOS_PMAX, "sc_mosaic: P=%d planes outside [1, %d]", a->P, MOS_PMAX);
  SC_REQUIRE(a->out_h >= 1 && a->out_w >= 1, "sc_mosaic: bad dims out %d x %d", a->out_h, a->out_w);
  SC_REQUIRE((long long)a->out_h * a->out_w < (1LL << 31), "sc_mosaic: %d x %d output pixels do not fit 31 bits", a->out_h, a->out_w);
  const int eb = a->elem_bytes;
  SC_REQUIRE(eb == 1 || eb == 2 || eb == 4 || eb == 8, "sc_mosaic: element width %d (1, 2, 4 or 8 bytes expected)", eb);
  SC_REQUIRE(a->resampling == SC_WARP_NEAREST || a->resampling == SC_WARP_BILINEAR, "sc_mosaic: resampling %d (0 = nearest, 1 = bilinear)",
             a->resampling);
  SC_REQUIRE(a->rule >= SC_MOSAIC_FIRST && a->rule <= SC_MOSAIC_BY_INDEX, "sc_mosaic: rule %d (0 first, 1 last, 2 max, 3 min, 4 mean, 5 by index)",
             a->rule);
  SC_REQUIRE(a->key_plane >= -1 && a->key_plane < a->P, "sc_mosaic: key_plane=%d outside [-1, %d)", a->key_plane, a->P);
  SC_REQUIRE((a->flags & ~SC_MOSAIC_KEY_FLOAT) == 0 && (a->flags == 0 || eb == 4 || eb == 8),
             "sc_mosaic: flags %d (SC_MOSAIC_KEY_FLOAT, and only with 4- or 8-byte elements)", a->flags);
  const bool bil = a->resampling == SC_WARP_BILINEAR, mean = a->rule == SC_MOSAIC_MEAN;
  const bool by_key = a->rule == SC_MOSAIC_MAX || a->rule == SC_MOSAIC_MIN;
  SC_REQUIRE(!bil || eb == 4, "sc_mosaic: bilinear resampling is defined for float32 planes, not %d-byte elements", eb);
  SC_REQUIRE(!(by_key || mean) || eb == 4, "sc_mosaic: the rules max, min and mean are defined for float32 planes, not %d-byte elements", eb);
  SC_REQUIRE(!by_key || a->key_plane >= 0, "sc_mosaic: the rules max and min need a key plane");
  SC_REQUIRE(!mean || a->P <= MOS_MEANP, "sc_mosaic: the rule mean takes at most %d planes per call, not %d", MOS_MEANP, a->P);
  SC_REQUIRE(!mean || !a->index, "sc_mosaic: the rule mean has no winner: index must be NULL");
  SC_REQUIRE(a->rule != SC_MOSAIC_BY_INDEX || (a->select && !a->count), "sc_mosaic: by index needs `select` and writes no count");
  SC_REQUIRE(a->out && a->sources && a->table, "sc_mosaic: null output, source array or table pointer");
  SC_REQUIRE((uintptr_t)a->out % eb == 0 && (uintptr_t)a->index % 4 == 0 && (uintptr_t)a->count % 4 == 0 && (uintptr_t)a->select % 4 == 0 &&
                 (uintptr_t)a->table % 8 == 0,
             "sc_mosaic: misaligned output, index, count, select or table pointer");
  MosD d;
  for (int i = 0; i < 6; ++i) {
    SC_REQUIRE(std::isfinite(a->dst_gt[i]), "sc_mosaic: destination geotransform term %d is not finite", i);
    d.gt[i] = a->dst_gt[i];
  }
  SC_REQUIRE(a->dst_gt[1] * a->dst_gt[5] - a->dst_gt[2] * a->dst_gt[4] != 0.0, "sc_mosaic: the destination geotransform is singular");
  SC_REQUIRE(a->dst_crs >= 0, "sc_mosaic: negative CRS code %d", a->dst_crs);
  d.dst_kind = 0;
  d.dst_lon0 = d.dst_fn = 0.0;
  for (int s = 0; s < a->N; ++s) {
    const sc_mosaic_source& q = a->sources[s];
    SC_REQUIRE(q.src_h >= 1 && q.src_w >= 1, "sc_mosaic: source %d is %d x %d", s, q.src_h, q.src_w);
    for (int i = 0; i < 6; ++i) SC_REQUIRE(std::isfinite(q.src_inv[i]), "sc_mosaic: source %d: geotransform term %d is not finite", s, i);
    SC_REQUIRE(q.src_inv[1] * q.src_inv[5] - q.src_inv[2] * q.src_inv[4] != 0.0, "sc_mosaic: source %d: the inverse geotransform is singular", s);
    if (q.src_crs != a->dst_crs) {                // equal codes (0 included): affine only
      double lon0, fn0;
      const int kd = crs_kind(a->dst_crs, d.dst_lon0, d.dst_fn), ks = crs_kind(q.src_crs, lon0, fn0);
      SC_REQUIRE(kd > 0 && ks > 0, "sc_mosaic: source %d: CRS pair %d -> %d (equal codes, else 4326 or 32601..32660 / 32701..32760 on both sides)",
                 s, a->dst_crs, q.src_crs);
      d.dst_kind = kd;
    }
    SC_REQUIRE(q.box[0] >= 0 && q.box[1] <= a->out_h && q.box[2] >= 0 && q.box[3] <= a->out_w,
               "sc_mosaic: source %d: box (%d, %d, %d, %d) outside the %d x %d grid", s, q.box[0], q.box[1], q.box[2], q.box[3], a->out_h, a->out_w);
    for (int p = 0; p < a->P; ++p) {
      SC_REQUIRE(q.src[p], "sc_mosaic: source %d: null plane %d", s, p);
      SC_REQUIRE((uintptr_t)q.src[p] % eb == 0, "sc_mosaic: source %d: plane %d is not aligned to its %d-byte elements", s, p, eb);
      SC_REQUIRE(q.row_stride[p] >= 0 && q.col_stride[p] >= 0, "sc_mosaic: source %d: negative stride of plane %d", s, p);
    }
  }
  krueger_wgs84(d.k);
  d.dst_crs = a->dst_crs;
  d.H = a->out_h; d.W = a->out_w; d.P = a->P; d.N = a->N; d.tiles_x = 0;
  d.rule = a->rule; d.key = a->key_plane; d.keyfloat = (a->flags & SC_MOSAIC_KEY_FLOAT) || by_key || mean;
  d.tab = static_cast<const sc_mosaic_source*>(a->table);
  d.out = a->out; d.index = a->index; d.count = a->count; d.select = a->select;
  for (int p = 0; p < MOS_PMAX; ++p) d.nod[p] = p < a->P ? a->nodata_bits[p] : 0;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemcpyAsync(a->table, a->sources, (size_t)a->N * sizeof(sc_mosaic_source), hipMemcpyHostToDevice, st) != hipSuccess) {
    sc_set_error("sc_mosaic: the copy of the source table failed");
    return SC_ERR_LAUNCH;
  }
  const int V = eb == 8 ? 2 : 4;
  const uintptr_t store = (uintptr_t)(V * eb < 16 ? V * eb : 16), istore = (uintptr_t)(4 * V);
  const bool vec = a->out_w % V == 0 && (uintptr_t)a->out % store == 0 && (uintptr_t)a->index % istore == 0 &&
                   (uintptr_t)a->count % istore == 0 && (uintptr_t)a->select % istore == 0;
  int rc;
  if (mean) rc = bil ? launch<uint32_t, 4, true, true>(d, vec, st) : launch<uint32_t, 4, false, true>(d, vec, st);
  else if (bil) rc = launch<uint32_t, 4, true, false>(d, vec, st);
  else if (eb == 1) rc = launch<uint8_t, 4, false, false>(d, vec, st);
  else if (eb == 2) rc = launch<uint16_t, 4, false, false>(d, vec, st);
  else if (eb == 4) rc = launch<uint32_t, 4, false, false>(d, vec, st);
  else rc = launch<uint64_t, 2, false, false>(d, vec, st);
  if (rc) return rc;
  SC_LAUNCH_OK("sc_mosaic");
  return SC_OK;
}
