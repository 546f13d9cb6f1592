// Per-component statistics of a label image (sc_component_stats): the plume catalogue behind starcop_amd/plumes.py.
// For N images, every component k (the pixels of value k, 1 <= k <= min(counts[n], M)) is reduced over up to 8 float32 planes
// and one uint8 mask.  Five launches, whatever the images hold; no floating-point atomics, no work-group waits on another:
//   init    : the four box columns of every row get the identities of min / max.
//   boxes   : one thread per pixel.  The bounding box by integer atomicMin / atomicMax -- only from pixels that can move a side
//             (row_min only where the pixel above carries another value, col_max only where the pixel to the right does, ..),
//             and only after a plain load says the side would move: a solid component issues atomics from its outline alone.
//   plan    : one work-group per image.  Every box is cut into row bands of `bh` rows; bh = max(32, ceil(sum of box heights /
//             extra)) with extra = ceil(H*W / 4096), so that the image has at most counts[n] + extra (component, band) items
//             whatever it holds.  An exclusive scan of the band counts gives each component its first item.
//   walk    : one wave per item.  It walks its band of the box in raster order at a fixed lane stride, keeps per-lane partials
//             (int64 counts and coordinate sums, fp64 sums in ascending raster order, max / min / first index of the max), folds
//             them with one xor butterfly and writes the item's record.
//   combine : one thread per output row folds the records of its component in band order and writes every output column;
//             rows at or above counts[n] are zero-filled.
// The band height depends on the image's own boxes, H and W only, the lane a pixel falls to on its box only: the order of every
// fp64 addition is fixed by the label image, so repeated calls, and an image alone or inside a batch, give identical bits.
// Work is proportional to the sum of the box areas (DESIGN section 26 has the worst case).
#include "sc_common.h"

#include <limits.h>

namespace {

constexpr int MAXP = SC_CSTATS_MAX_PLANES;
constexpr int BAND_ROWS = 32;          // smallest band height
constexpr int EXTRA_PX = 4096;         // one spare item per this many pixels of the image

// one (component, band) record
struct PlaneRec {
  long long n_finite;
  double sum;
  float mx, mn;
  long long argmax;                    // raster index of the first maximum; INT_MAX when the band holds no finite value
};
struct ItemRec {
  long long area, sum_row, sum_col, n_other, first;
};
__host__ __device__ inline size_t item_bytes(int P) { return sizeof(ItemRec) + (size_t)P * sizeof(PlaneRec); }

struct StatsP {
  const int* labels; const int* counts;
  int N, H, W, M, P, cap;              // cap: item slots per image = M + extra
  int min_band;                        // smallest band height (BAND_ROWS here; sc_component_radial cuts finer)
  long long extra;
  const float* plane[MAXP]; long long plane_stride[MAXP];
  const unsigned char* other; long long other_stride;
  long long* area; int* row_min; int* row_max; int* col_min; int* col_max;
  long long* sum_row; long long* sum_col; long long* first_pixel; long long* n_other;
  long long* n_finite; double* sum; float* mx; float* mn; long long* argmax;
  int* off;                            // [N][M + 1] first item of every component, then the image's item count
  int* bandh;                          // [N] band height
  unsigned char* items;                // [N][cap] records of item_bytes(P)
};

__device__ __forceinline__ int n_components(const StatsP& p, int n) { return min(max(p.counts[n], 0), p.M); }
__device__ __forceinline__ int ld(const int* q) { return __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(256) void k_cs_init(const StatsP p) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)p.N * p.M) return;
  p.row_min[i] = INT_MAX; p.col_min[i] = INT_MAX; p.row_max[i] = -1; p.col_max[i] = -1;
}

__global__ __launch_bounds__(256) void k_cs_boxes(const StatsP p) {
  const int n = blockIdx.y, H = p.H, W = p.W;
  const long long i64 = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i64 >= (long long)H * W) return;
  const long long i = (int)i64;                                // H*W < 2^31: the division below is a 32-bit one
  const int* L = p.labels + (size_t)n * H * W;
  const int k = L[i];
  if (k < 1 || k > n_components(p, n)) return;                 // background, and values that name no row
  const int r = (int)i / W, c = (int)i - r * W;
  const size_t row = (size_t)n * p.M + (k - 1);
  if ((r == 0 || L[i - W] != k) && r < ld(p.row_min + row)) atomicMin(p.row_min + row, r);
  if ((r == H - 1 || L[i + W] != k) && r > ld(p.row_max + row)) atomicMax(p.row_max + row, r);
  if ((c == 0 || L[i - 1] != k) && c < ld(p.col_min + row)) atomicMin(p.col_min + row, c);
  if ((c == W - 1 || L[i + 1] != k) && c > ld(p.col_max + row)) atomicMax(p.col_max + row, c);
}

__device__ __forceinline__ int n_bands(int h, int bh) { return (int)(((long long)h + bh - 1) / bh); }

// band height of the image, then the exclusive scan of the band counts (the scan of k_cc_scan in labels.hip)
__global__ __launch_bounds__(256) void k_cs_plan(const StatsP p) {
  __shared__ long long tot;
  __shared__ int part[256];
  const int n = blockIdx.x, tid = threadIdx.x;
  const int cnt = n_components(p, n);
  const int* rmin = p.row_min + (size_t)n * p.M;
  const int* rmax = p.row_max + (size_t)n * p.M;
  int* off = p.off + (size_t)n * (p.M + 1);
  if (tid == 0) tot = 0;
  __syncthreads();
  long long hs = 0;
  for (int k = tid; k < cnt; k += 256)
    if (rmax[k] >= rmin[k]) hs += rmax[k] - rmin[k] + 1;
  atomicAdd(reinterpret_cast<unsigned long long*>(&tot), (unsigned long long)hs);      // integer: any order, one value
  __syncthreads();
  const long long need = (tot + p.extra - 1) / p.extra;
  const long long low = p.min_band, top = p.H > low ? p.H : low;      // a band of H rows is the whole box already
  const int bh = (int)(need < low ? low : (need > top ? top : need));
  const int per = (cnt + 255) / 256, k0 = min(cnt, tid * per), k1 = min(cnt, k0 + per);
  int s = 0;
  for (int k = k0; k < k1; ++k)
    if (rmax[k] >= rmin[k]) s += n_bands(rmax[k] - rmin[k] + 1, bh);
  part[tid] = s;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const int v = tid >= o ? part[tid - o] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  int acc = part[tid] - s;
  for (int k = k0; k < k1; ++k) {
    off[k] = acc;
    if (rmax[k] >= rmin[k]) acc += n_bands(rmax[k] - rmin[k] + 1, bh);
  }
  if (tid == 255) off[cnt] = min(part[255], p.cap);             // <= cnt + extra <= cap by the choice of bh
  if (tid == 0) p.bandh[n] = bh;
}

__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
// (value, first index) of the larger value; of equal values the one at the smaller index
__device__ __forceinline__ void take_max(float& mx, int& am, float omx, int oam) {
  if (omx > mx || (omx == mx && oam < am)) { mx = omx; am = oam; }
}
__device__ __forceinline__ long long wave_sum_ll(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void k_cs_walk(const StatsP p) {
  const int n = blockIdx.y, lane = threadIdx.x & 63;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);            // item of this wave; whole waves leave together
  const int cnt = n_components(p, n);
  const int* off = p.off + (size_t)n * (p.M + 1);
  if (w >= off[cnt]) return;
  int lo = 0, hi = cnt - 1;                                     // the last k with off[k] <= w (components without pixels share
  while (lo < hi) {                                             // the offset of their successor and are never the last)
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= w) lo = mid; else hi = mid - 1;
  }
  const int k = lo, W = p.W;
  const size_t row = (size_t)n * p.M + k;
  const int bh = p.bandh[n];
  const int c0 = p.col_min[row], c1 = p.col_max[row];
  const long long r0 = p.row_min[row] + (long long)(w - off[k]) * bh, r1 = min((long long)p.row_max[row] + 1, r0 + bh);
  // a box narrower than the wave puts several rows side by side: pw = the power of two >= its width
  const int bw = c1 - c0 + 1;
  int sh = 6;
  while (sh > 0 && (1 << (sh - 1)) >= bw) --sh;
  const int pw = 1 << sh, rows_per_step = 64 >> sh;
  const int* L = p.labels + (size_t)n * p.H * W;
  const unsigned char* other = p.other ? p.other + (long long)n * p.other_stride : nullptr;
  const int P = p.P, lab = k + 1;

  long long area = 0, srow = 0, scol = 0, noth = 0;
  int first = INT_MAX;
  long long nf[MAXP]; double sm[MAXP]; float mx[MAXP], mn[MAXP]; int am[MAXP];
#pragma unroll
  for (int q = 0; q < MAXP; ++q) { nf[q] = 0; sm[q] = 0.0; mx[q] = -__builtin_inff(); mn[q] = __builtin_inff(); am[q] = INT_MAX; }

  for (long long r = r0 + (lane >> sh); r < r1; r += rows_per_step) {     // 64-bit: r + 64 and c + 64 may pass 2^31
    for (long long c = c0 + (lane & (pw - 1)); c <= c1; c += pw) {
      const int i = (int)(r * W + c);
      if (L[i] != lab) continue;
      ++area; srow += r; scol += c;
      first = min(first, i);
      if (other && other[i]) ++noth;
#pragma unroll
      for (int q = 0; q < MAXP; ++q) {
        if (q < P) {
          const float v = p.plane[q][(long long)n * p.plane_stride[q] + i];
          if (finite_f(v)) {
            ++nf[q]; sm[q] += (double)v;
            if (v > mx[q]) { mx[q] = v; am[q] = i; }            // i ascends along a lane: the first maximum stays
            if (v < mn[q]) mn[q] = v;
          }
        }
      }
    }
  }
  area = wave_sum_ll(area); srow = wave_sum_ll(srow); scol = wave_sum_ll(scol); noth = wave_sum_ll(noth);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o, 64));
  unsigned char* rec = p.items + ((size_t)n * p.cap + w) * item_bytes(P);
  if (lane == 0) {
    ItemRec* it = reinterpret_cast<ItemRec*>(rec);
    it->area = area; it->sum_row = srow; it->sum_col = scol; it->n_other = noth; it->first = first;
  }
  PlaneRec* pr = reinterpret_cast<PlaneRec*>(rec + sizeof(ItemRec));
#pragma unroll
  for (int q = 0; q < MAXP; ++q) {
    if (q < P) {
      const long long c_ = wave_sum_ll(nf[q]);
      const double s_ = wave_sum_d(sm[q]);                      // one fixed butterfly over the per-lane sums
      float m_ = mx[q], l_ = mn[q]; int a_ = am[q];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        take_max(m_, a_, __shfl_xor(m_, o, 64), __shfl_xor(a_, o, 64));
        const float ol = __shfl_xor(l_, o, 64);
        if (ol < l_) l_ = ol;
      }
      if (lane == 0) { pr[q].n_finite = c_; pr[q].sum = s_; pr[q].mx = m_; pr[q].mn = l_; pr[q].argmax = a_; }
    }
  }
}

__global__ __launch_bounds__(256) void k_cs_combine(const StatsP p) {
  const int n = blockIdx.y;
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= p.M) return;
  const size_t row = (size_t)n * p.M + m;
  const int P = p.P;
  if (m >= n_components(p, n)) {
    p.area[row] = 0; p.row_min[row] = 0; p.row_max[row] = 0; p.col_min[row] = 0; p.col_max[row] = 0;
    p.sum_row[row] = 0; p.sum_col[row] = 0; p.first_pixel[row] = 0; p.n_other[row] = 0;
    for (int q = 0; q < P; ++q) {
      const size_t o = row * P + q;
      p.n_finite[o] = 0; p.sum[o] = 0.0; p.mx[o] = 0.f; p.mn[o] = 0.f; p.argmax[o] = 0;
    }
    return;
  }
  const int* off = p.off + (size_t)n * (p.M + 1);
  const int i0 = off[m], i1 = off[m + 1];
  const size_t ib = item_bytes(P);
  const unsigned char* base = p.items + (size_t)n * p.cap * ib;
  long long area = 0, srow = 0, scol = 0, noth = 0, first = INT_MAX;
  for (int i = i0; i < i1; ++i) {
    const ItemRec* it = reinterpret_cast<const ItemRec*>(base + (size_t)i * ib);
    area += it->area; srow += it->sum_row; scol += it->sum_col; noth += it->n_other;
    first = it->first < first ? it->first : first;
  }
  p.area[row] = area; p.sum_row[row] = srow; p.sum_col[row] = scol; p.n_other[row] = noth;
  p.first_pixel[row] = area ? first : -1;
  if (!area) { p.row_min[row] = 0; p.row_max[row] = 0; p.col_min[row] = 0; p.col_max[row] = 0; }   // a value no pixel carries
  for (int q = 0; q < P; ++q) {
    long long nf = 0; double s = 0.0; float mx = -__builtin_inff(), mn = __builtin_inff(); int am = INT_MAX;
    for (int i = i0; i < i1; ++i) {                               // band order
      const PlaneRec* pr = reinterpret_cast<const PlaneRec*>(base + (size_t)i * ib + sizeof(ItemRec)) + q;
      nf += pr->n_finite; s += pr->sum;
      take_max(mx, am, pr->mx, (int)pr->argmax);
      if (pr->mn < mn) mn = pr->mn;
    }
    const size_t o = row * P + q;
    p.n_finite[o] = nf;
    p.sum[o] = nf ? s : 0.0;
    p.mx[o] = nf ? mx : __builtin_nanf("");
    p.mn[o] = nf ? mn : __builtin_nanf("");
    p.argmax[o] = nf ? am : -1;
  }
}

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
inline long long extra_items(int H, int W) { return ((long long)H * W + EXTRA_PX - 1) / EXTRA_PX; }
bool dims_ok(int N, int H, int W, int M, int P) {
  return N > 0 && H > 0 && W > 0 && N <= 65535 && (long long)H * W < (1ll << 31) && M >= 0 && P >= 0 && P <= MAXP &&
         (long long)N * (M + 1ll) < (1ll << 31) && M + extra_items(H, W) < (1ll << 31);
}
size_t off_bytes(int N, int M) { return align256((size_t)N * (M + 1) * 4); }
size_t work_bytes_of(int N, int H, int W, int M, int P) {
  return off_bytes(N, M) + align256((size_t)N * 4) + align256((size_t)N * (size_t)(M + extra_items(H, W)) * item_bytes(P));
}

}  // namespace

extern "C" size_t sc_component_stats_workspace_bytes(int N, int H, int W, int M, int P) {
  if (!dims_ok(N, H, W, M, P)) return 0;
  return work_bytes_of(N, H, W, M, P);
}

extern "C" int sc_component_stats(const sc_cstats_args* a, void* work, size_t work_bytes, sc_stream stream) {
  SC_REQUIRE(a, "sc_component_stats: null arguments");
  SC_REQUIRE(dims_ok(a->N, a->H, a->W, a->M, a->P),
             "sc_component_stats: bad dims N=%d H=%d W=%d M=%d P=%d (N <= 65535, H*W < 2^31, N*(M+1) < 2^31, P <= %d)", a->N, a->H,
             a->W, a->M, a->P, MAXP);
  SC_REQUIRE(a->labels && a->counts, "sc_component_stats: null labels or counts");
  const long long HW = (long long)a->H * a->W;
  for (int q = 0; q < a->P; ++q) {
    SC_REQUIRE(a->plane[q], "sc_component_stats: plane %d is null", q);
    SC_REQUIRE(a->N == 1 || a->plane_stride[q] >= HW, "sc_component_stats: plane %d stride %lld overlaps %d x %d images", q,
               (long long)a->plane_stride[q], a->H, a->W);
  }
  SC_REQUIRE(!a->other || a->N == 1 || a->other_stride >= HW, "sc_component_stats: other stride %lld overlaps %d x %d images",
             (long long)a->other_stride, a->H, a->W);
  if (a->M == 0) return SC_OK;                                    // no rows to write
  SC_REQUIRE(a->area && a->row_min && a->row_max && a->col_min && a->col_max && a->sum_row && a->sum_col && a->first_pixel &&
                 a->n_other, "sc_component_stats: null output column");
  SC_REQUIRE(a->P == 0 || (a->n_finite && a->sum && a->max && a->min && a->argmax), "sc_component_stats: null plane output column");
  SC_REQUIRE(work && work_bytes >= work_bytes_of(a->N, a->H, a->W, a->M, a->P), "sc_component_stats: workspace %zu < %zu bytes",
             work_bytes, work_bytes_of(a->N, a->H, a->W, a->M, a->P));
  hipStream_t st = (hipStream_t)stream;
  StatsP p{};
  p.labels = a->labels; p.counts = a->counts;
  p.N = a->N; p.H = a->H; p.W = a->W; p.M = a->M; p.P = a->P;
  p.extra = extra_items(a->H, a->W); p.cap = (int)(a->M + p.extra); p.min_band = BAND_ROWS;
  for (int q = 0; q < a->P; ++q) { p.plane[q] = a->plane[q]; p.plane_stride[q] = a->plane_stride[q]; }
  p.other = a->other; p.other_stride = a->other_stride;
  p.area = (long long*)a->area; p.row_min = a->row_min; p.row_max = a->row_max; p.col_min = a->col_min; p.col_max = a->col_max;
  p.sum_row = (long long*)a->sum_row; p.sum_col = (long long*)a->sum_col; p.first_pixel = (long long*)a->first_pixel;
  p.n_other = (long long*)a->n_other;
  p.n_finite = (long long*)a->n_finite; p.sum = a->sum; p.mx = a->max; p.mn = a->min; p.argmax = (long long*)a->argmax;
  char* wp = static_cast<char*>(work);
  p.off = reinterpret_cast<int*>(wp);
  p.bandh = reinterpret_cast<int*>(wp + off_bytes(a->N, a->M));
  p.items = reinterpret_cast<unsigned char*>(wp + off_bytes(a->N, a->M) + align256((size_t)a->N * 4));
  const long long rows = (long long)a->N * a->M;
  hipLaunchKernelGGL(k_cs_init, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, p);
  SC_LAUNCH_OK("k_cs_init");
  hipLaunchKernelGGL(k_cs_boxes, dim3((unsigned)((HW + 255) / 256), a->N), dim3(256), 0, st, p);
  SC_LAUNCH_OK("k_cs_boxes");
  hipLaunchKernelGGL(k_cs_plan, dim3(a->N), dim3(256), 0, st, p);
  SC_LAUNCH_OK("k_cs_plan");
  hipLaunchKernelGGL(k_cs_walk, dim3((unsigned)((p.cap + 3) / 4), a->N), dim3(256), 0, st, p);
  SC_LAUNCH_OK("k_cs_walk");
  hipLaunchKernelGGL(k_cs_combine, dim3((unsigned)((a->M + 255) / 256), a->N), dim3(256), 0, st, p);
  SC_LAUNCH_OK("k_cs_combine");
  return SC_OK;
}

// Radial profiles per component (sc_component_radial): the fetch profiles behind starcop_amd/plumes.py: component_radial.
// The boxes come from sc_component_stats, so three launches do: the plan above (k_cs_plan with a lower floor for the band height:
// band height and first item of every component from the boxes), then
//   walk    : one wave per (component, band) item, four to a work-group.  The wave steps through its band of the box in raster
//             order, 64 pixels a step.  Every lane finds the bin of its pixel (the smallest j with d2 <= edge2[j], a binary search
//             of the edges in LDS).  Then, while lanes remain: the bin of the first remaining lane is broadcast, ONE fixed xor
//             butterfly sums `lane in that bin ? value : 0.0`, and lane 0 adds the result to the wave's own fp64 sum of that bin in
//             LDS (the count is the popcount of the ballot).  Along a row a 64-pixel run crosses few bins, so the loop is short.
//             The moments and the largest d2 are per-lane integers folded by a butterfly at the end.
//   combine : one thread per (row, bin) folds the records of its component in band order.
// Which lanes a bin's butterfly selects, the order in which the bins of a step are taken (by their first lane) and the order of
// the steps depend on the label image, the box, the origin, the edges and which values are finite -- not on the values, the batch
// or the call: every fp64 sum is a fixed expression tree, so the bits repeat.
namespace {

constexpr int MAXK = SC_CRADIAL_MAX_BINS;
// Bands of 4 rows and one spare item per 512 pixels: a plume mask has a few hundred boxes, and a wave's step is a chain of a
// load, a search and a few butterflies -- many short waves hide that latency, few long ones do not.  The bound of the plan holds
// for any floor and any spare count: sum_k ceil(h_k / bh) <= counts[n] + extra with bh >= ceil(sum of heights / extra).
constexpr int RAD_BAND_ROWS = 4;
constexpr int RAD_EXTRA_PX = 512;
inline long long rad_extra_items(int H, int W) { return ((long long)H * W + RAD_EXTRA_PX - 1) / RAD_EXTRA_PX; }

struct RadRec { long long d2_max, sum_rr, sum_cc, sum_rc; };
struct BinRec { long long n; double s; };
__host__ __device__ inline size_t rad_item_bytes(int K) { return sizeof(RadRec) + (size_t)(K + 1) * sizeof(BinRec); }

struct RadP {
  const int* labels; const int* counts;
  int N, H, W, M, K, cap;
  const int* row_min; const int* row_max; const int* col_min; const int* col_max; const int* origin;
  const float* plane; long long plane_stride;
  int edge2[MAXK];
  long long* bin_count; double* bin_sum; long long* d2_max; long long* sum_rr; long long* sum_cc; long long* sum_rc;
  const int* off; const int* bandh; unsigned char* items;
};

__device__ __forceinline__ int n_components(const RadP& p, int n) { return min(max(p.counts[n], 0), p.M); }
// items of image n: what the plan counted, inside the slots there are whatever boxes the caller passed
__device__ __forceinline__ int n_items(const RadP& p, int n, int cnt) { return min(max(p.off[(size_t)n * (p.M + 1) + cnt], 0), p.cap); }

__global__ __launch_bounds__(256) void k_cr_walk(const RadP p) {
  __shared__ int s_edge[MAXK];
  __shared__ double s_sum[4][MAXK + 1];
  __shared__ long long s_cnt[4][MAXK + 1];
  const int n = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int w = blockIdx.x * 4 + wv;                              // item of this wave; no wave leaves before the last barrier
  const int K = p.K, W = p.W;
  if ((int)threadIdx.x < K) s_edge[threadIdx.x] = p.edge2[threadIdx.x];
  for (int j = lane; j <= K; j += 64) { s_sum[wv][j] = 0.0; s_cnt[wv][j] = 0; }
  __syncthreads();
  const int cnt = n_components(p, n);
  const int* off = p.off + (size_t)n * (p.M + 1);
  const bool live = w < n_items(p, n, cnt);
  int k = 0;
  if (live) {
    int lo = 0, hi = cnt - 1;                                     // the last k with off[k] <= w, as k_cs_walk finds it
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (off[mid] <= w) lo = mid; else hi = mid - 1;
    }
    k = lo;
  }
  const size_t row = (size_t)n * p.M + k;
  const int bh = p.bandh[n];
  const long long o_r = p.origin[2 * row], o_c = p.origin[2 * row + 1];
  // the box, cut to the image: a box that is not the component's own gives other numbers, never another address
  const int c0 = max(p.col_min[row], 0), c1 = min(p.col_max[row], W - 1);
  long long r0 = p.row_min[row] + (long long)(w - off[k]) * bh;
  long long r1 = min(min((long long)p.row_max[row] + 1, r0 + bh), (long long)p.H);
  r0 = max(r0, 0ll);
  if (!live || o_r < 0) r1 = r0;                                  // a skipped plume leaves a record of zeros
  const int bw = c1 - c0 + 1;
  int sh = 6;
  while (sh > 0 && (1 << (sh - 1)) >= bw) --sh;
  const int pw = 1 << sh, rows_per_step = 64 >> sh;
  const int* L = p.labels + (size_t)n * p.H * W;
  const float* plane = p.plane + (long long)n * p.plane_stride;
  const int lab = k + 1;

  long long d2m = -1, srr = 0, scc = 0, src = 0;
  for (long long rb = r0; rb < r1; rb += rows_per_step) {          // both loops run the same number of times in every lane
    for (long long cb = c0; cb <= c1; cb += pw) {
      const long long r = rb + (lane >> sh), c = cb + (lane & (pw - 1));
      int bin = -1;
      float v = 0.f;
      if (r < r1 && c <= c1) {
        const int i = (int)(r * W + c);
        const int li = L[i];
        v = plane[i];                                             // with the label, not after it: one load latency per step
        if (li == lab) {
          const long long dr = r - o_r, dc = c - o_c, d2 = dr * dr + dc * dc;
          d2m = d2 > d2m ? d2 : d2m;
          srr += r * r; scc += c * c; src += r * c;
          if (finite_f(v)) {
            int lo = 0, hi = K;                                   // the smallest j with d2 <= edge2[j]; K beyond the last edge
            while (lo < hi) {
              const int mid = (lo + hi) >> 1;
              if (d2 > (long long)s_edge[mid]) lo = mid + 1; else hi = mid;
            }
            bin = lo;
          }
        }
      }
      unsigned long long rem = __ballot(bin >= 0);
      while (rem) {                                               // one round per distinct bin of the step, by first lane
        const int b = __shfl(bin, __ffsll((long long)rem) - 1, 64);
        const bool sel = bin == b;
        const unsigned long long m = __ballot(sel);
        const double s = wave_sum_d(sel ? (double)v : 0.0);
        if (lane == 0) { s_sum[wv][b] += s; s_cnt[wv][b] += __popcll(m); }
        rem &= ~m;
      }
    }
  }
  srr = wave_sum_ll(srr); scc = wave_sum_ll(scc); src = wave_sum_ll(src);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const long long od = __shfl_xor(d2m, o, 64);
    d2m = od > d2m ? od : d2m;
  }
  __syncthreads();                                                // lane 0's sums, before the other lanes read them
  if (!live) return;
  unsigned char* rec = p.items + ((size_t)n * p.cap + w) * rad_item_bytes(K);
  if (lane == 0) {
    RadRec* it = reinterpret_cast<RadRec*>(rec);
    it->d2_max = d2m; it->sum_rr = srr; it->sum_cc = scc; it->sum_rc = src;
  }
  BinRec* br = reinterpret_cast<BinRec*>(rec + sizeof(RadRec));
  for (int j = lane; j <= K; j += 64) { br[j].n = s_cnt[wv][j]; br[j].s = s_sum[wv][j]; }
}

__global__ __launch_bounds__(256) void k_cr_combine(const RadP p) {
  const int n = blockIdx.y, K1 = p.K + 1;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)p.M * K1) return;
  const int m = (int)(t / K1), j = (int)(t - (long long)m * K1);
  const size_t row = (size_t)n * p.M + m;
  const int cnt = n_components(p, n);
  int i0 = 0, i1 = 0;
  if (m < cnt) {
    const int* off = p.off + (size_t)n * (p.M + 1);
    const int tot = n_items(p, n, cnt);
    i0 = min(max(off[m], 0), tot); i1 = min(max(off[m + 1], i0), tot);
  }
  const size_t ib = rad_item_bytes(p.K);
  const unsigned char* base = p.items + (size_t)n * p.cap * ib;
  long long c = 0; double s = 0.0;
  for (int i = i0; i < i1; ++i) {                                 // band order
    const BinRec* br = reinterpret_cast<const BinRec*>(base + (size_t)i * ib + sizeof(RadRec)) + j;
    c += br->n; s += br->s;
  }
  p.bin_count[row * K1 + j] = c; p.bin_sum[row * K1 + j] = s;
  if (j != 0) return;
  long long d2m = -1, srr = 0, scc = 0, src = 0;
  for (int i = i0; i < i1; ++i) {
    const RadRec* it = reinterpret_cast<const RadRec*>(base + (size_t)i * ib);
    d2m = it->d2_max > d2m ? it->d2_max : d2m; srr += it->sum_rr; scc += it->sum_cc; src += it->sum_rc;
  }
  p.d2_max[row] = d2m; p.sum_rr[row] = srr; p.sum_cc[row] = scc; p.sum_rc[row] = src;
}

bool rad_dims_ok(int N, int H, int W, int M) {
  return dims_ok(N, H, W, M, 0) && H <= SC_CRADIAL_MAX_SIDE && W <= SC_CRADIAL_MAX_SIDE && (long long)M * (MAXK + 1) < (1ll << 31) &&
         M + rad_extra_items(H, W) < (1ll << 31);
}
size_t rad_work_bytes_of(int N, int H, int W, int M, int K) {
  return off_bytes(N, M) + align256((size_t)N * 4) + align256((size_t)N * (size_t)(M + rad_extra_items(H, W)) * rad_item_bytes(K));
}

}  // namespace

extern "C" size_t sc_component_radial_workspace_bytes(int N, int H, int W, int M, int K) {
  if (!rad_dims_ok(N, H, W, M) || K < 1 || K > MAXK) return 0;
  return rad_work_bytes_of(N, H, W, M, K);
}

extern "C" int sc_component_radial(const sc_cradial_args* a, void* work, size_t work_bytes, sc_stream stream) {
  SC_REQUIRE(a, "sc_component_radial: null arguments");
  SC_REQUIRE(rad_dims_ok(a->N, a->H, a->W, a->M),
             "sc_component_radial: bad dims N=%d H=%d W=%d M=%d (N <= 65535, H, W <= %d, H*W < 2^31, N*(M+1) < 2^31, M*%d < 2^31)",
             a->N, a->H, a->W, a->M, SC_CRADIAL_MAX_SIDE, MAXK + 1);
  SC_REQUIRE(a->K >= 1 && a->K <= MAXK, "sc_component_radial: K=%d bin edges (1 .. %d)", a->K, MAXK);
  SC_REQUIRE(a->edge2[0] >= 0, "sc_component_radial: edge2[0] = %d is negative", a->edge2[0]);
  for (int j = 1; j < a->K; ++j)
    SC_REQUIRE(a->edge2[j] > a->edge2[j - 1], "sc_component_radial: edge2 must increase strictly: edge2[%d] = %d, edge2[%d] = %d",
               j - 1, a->edge2[j - 1], j, a->edge2[j]);
  SC_REQUIRE(a->labels && a->counts, "sc_component_radial: null labels or counts");
  SC_REQUIRE(a->plane, "sc_component_radial: null plane");
  SC_REQUIRE(a->N == 1 || a->plane_stride >= (long long)a->H * a->W, "sc_component_radial: plane stride %lld overlaps %d x %d images",
             (long long)a->plane_stride, a->H, a->W);
  if (a->M == 0) return SC_OK;                                    // no rows to write
  SC_REQUIRE(a->row_min && a->row_max && a->col_min && a->col_max && a->origin, "sc_component_radial: null box column or origin");
  SC_REQUIRE(a->bin_count && a->bin_sum && a->d2_max && a->sum_rr && a->sum_cc && a->sum_rc, "sc_component_radial: null output column");
  SC_REQUIRE(work && work_bytes >= rad_work_bytes_of(a->N, a->H, a->W, a->M, a->K), "sc_component_radial: workspace %zu < %zu bytes",
             work_bytes, rad_work_bytes_of(a->N, a->H, a->W, a->M, a->K));
  hipStream_t st = (hipStream_t)stream;
  char* wp = static_cast<char*>(work);
  StatsP sp{};                                                    // what k_cs_plan reads: the boxes, and where its plan goes
  sp.counts = a->counts; sp.N = a->N; sp.H = a->H; sp.W = a->W; sp.M = a->M;
  sp.extra = rad_extra_items(a->H, a->W); sp.cap = (int)(a->M + sp.extra); sp.min_band = RAD_BAND_ROWS;
  sp.row_min = const_cast<int*>(a->row_min); sp.row_max = const_cast<int*>(a->row_max);
  sp.off = reinterpret_cast<int*>(wp);
  sp.bandh = reinterpret_cast<int*>(wp + off_bytes(a->N, a->M));
  RadP p{};
  p.labels = a->labels; p.counts = a->counts;
  p.N = a->N; p.H = a->H; p.W = a->W; p.M = a->M; p.K = a->K; p.cap = sp.cap;
  p.row_min = a->row_min; p.row_max = a->row_max; p.col_min = a->col_min; p.col_max = a->col_max; p.origin = a->origin;
  p.plane = a->plane; p.plane_stride = a->plane_stride;
  for (int j = 0; j < a->K; ++j) p.edge2[j] = a->edge2[j];
  p.bin_count = (long long*)a->bin_count; p.bin_sum = a->bin_sum; p.d2_max = (long long*)a->d2_max;
  p.sum_rr = (long long*)a->sum_rr; p.sum_cc = (long long*)a->sum_cc; p.sum_rc = (long long*)a->sum_rc;
  p.off = sp.off; p.bandh = sp.bandh;
  p.items = reinterpret_cast<unsigned char*>(wp + off_bytes(a->N, a->M) + align256((size_t)a->N * 4));
  hipLaunchKernelGGL(k_cs_plan, dim3(a->N), dim3(256), 0, st, sp);
  SC_LAUNCH_OK("k_cs_plan");
  hipLaunchKernelGGL(k_cr_walk, dim3((unsigned)((p.cap + 3) / 4), a->N), dim3(256), 0, st, p);
  SC_LAUNCH_OK("k_cr_walk");
  const long long cells = (long long)a->M * (a->K + 1);
  hipLaunchKernelGGL(k_cr_combine, dim3((unsigned)((cells + 255) / 256), a->N), dim3(256), 0, st, p);
  SC_LAUNCH_OK("k_cr_combine");
  return SC_OK;
}
