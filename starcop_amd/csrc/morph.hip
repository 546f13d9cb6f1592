// Exact Euclidean distance transform of binary images and what follows from it: dilation / erosion by a disc (a threshold on
// the squared distance) and the sieve's gather (starcop_amd/morphology.py).  Separable min-plus transform, integers throughout.
//   column pass : g(h, w) = vertical distance to the nearest target of column w (SENT where the column has none), uint16.
//       Rows are cut into bands of 64: k_edt_bits packs the targets of every (band, column) into one 64-bit word (the only read
//       of the mask), k_edt_carry walks the bands of a column once for the nearest target above and below every band, and
//       k_edt_cols derives the 64 values of a (band, column) from its word and the two carries with clz / ctz -- no sweep, and
//       H / 64 times the lanes of a column-per-lane sweep.
//   row pass    : d2(h, x) = min_i (x - i)^2 + g(h, i)^2, one of
//       window   (cap known, R = floor(sqrt(cap)) <= SC_EDT_WINDOW_MAX_R): a work-group stages g^2 of 256 pixels of a row plus
//                an R-wide halo in LDS, every lane takes the minimum over |x - i| <= R.  Exact at or below the cap, anything
//                above the cap is FAR anyway.
//       envelope (unbounded, or a larger cap): the lower envelope of the parabolas of a row (Meijster's integer form of
//                Felzenszwalb-Huttenlocher), one row per lane over the TRANSPOSED g, so the lanes of a wave read and write
//                neighbouring addresses; the stack of a row lives in the workspace, its top in registers.  Work O(W) per row
//                whatever the distances.  A transposing kernel writes the outputs.
// The epilogue of the last pass writes any of dist2 / dist / within.  No floating-point atomics, no atomics at all; every value
// is a function of the image alone: two calls give identical bytes.
//
// sc_edt_nearest is the same two passes keeping the arg-min beside the minimum (the feature transform): the row passes are
// templated on their parameter block, EdtP for sc_edt (the instantiations sc_edt launches do no more than before) and NearP,
// which makes the window remember the column that won (left to right, replaced on < only: the smallest column among equals) and
// the envelope write the column of the parabola it evaluates (its intersection abscissa is the first column where the LATER
// parabola is strictly lower and its pop test keeps the earlier one on equality: the smallest column again).  The epilogue
// recomputes the row of the target from the band word and carries of (band(h), winning column), the upper target on a tie, and
// gathers up to SC_EDT_NEAREST_MAX_PLANES planes of 4-byte words there.
#include <type_traits>

#include "sc_common.h"

namespace {

constexpr int BH = 64;                       // rows per band of the column pass
constexpr unsigned SENT = 0xFFFFu;           // g of a column without a target (H <= 32767: real values stay below)
constexpr int BIG2 = 0x3FFFFFFF;             // "g^2" of such a column in the window pass: above every cap, and + R^2 cannot overflow
constexpr int SEG = 256;                     // pixels of a row per work-group of the window pass
constexpr int FAR_ = SC_EDT_FAR;

struct EdtP {
  const unsigned char* mask; long long sn, sh, sw;
  int N, H, W, invert, nb, Hp;
  unsigned long long* bits;                  // [N][nb][W]
  int* above; int* below;                    // [N][nb][W] row of the nearest target above / below the band, -1 for none
  unsigned short* g;                         // [N][H][W], or transposed [N][W][Hp]
  unsigned* stk;                             // [N][W][Hp] envelope stack below its top: t << 16 | s
  int* d2t;                                  // [N][W][Hp] envelope result, transposed
  int R, max_dist2, thresh2, negate;
  double pixel_size;
  int* dist2; float* dist; unsigned char* within;
};

// sc_edt_nearest: the same passes, and what the arg-min needs on top
struct NearP : EdtP {
  unsigned short* colt;                      // [N][W][Hp] envelope: column of the winning parabola, transposed beside d2t
  int* index;                                // [N][H][W] row_t * W + col_t, -1 where dist2 is FAR
  int np;
  const unsigned* src[SC_EDT_NEAREST_MAX_PLANES];
  long long ss[SC_EDT_NEAREST_MAX_PLANES];   // words between the images of a source plane
  unsigned* dst[SC_EDT_NEAREST_MAX_PLANES];
};

__device__ __forceinline__ void edt_store(const EdtP& p, size_t o, int d2) {
  if (p.within) p.within[o] = (d2 <= p.thresh2) != (p.negate != 0);
  if (p.max_dist2 > 0 && d2 > p.max_dist2) d2 = FAR_;
  if (p.dist2) p.dist2[o] = d2;
  if (p.dist) p.dist[o] = d2 == FAR_ ? __builtin_inff() : (float)(sqrt((double)d2) * p.pixel_size);
}

__global__ __launch_bounds__(256) void k_edt_bits(const EdtP p) {
  const int w = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y, n = blockIdx.z;
  if (w >= p.W) return;
  const unsigned char* m = p.mask + (long long)n * p.sn + (long long)w * p.sw;
  const int h0 = b * BH, rows = min(BH, p.H - h0);
  unsigned long long bits = 0;
  for (int r = 0; r < rows; ++r)
    if ((m[(long long)(h0 + r) * p.sh] != 0) != (p.invert != 0)) bits |= 1ull << r;
  p.bits[((size_t)n * p.nb + b) * p.W + w] = bits;
}

__global__ __launch_bounds__(256) void k_edt_carry(const EdtP p) {
  const int w = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;
  if (w >= p.W) return;
  const size_t base = (size_t)n * p.nb * p.W + w;
  int last = -1;
  for (int b = 0; b < p.nb; ++b) {
    const size_t o = base + (size_t)b * p.W;
    p.above[o] = last;
    const unsigned long long bits = p.bits[o];
    if (bits) last = b * BH + 63 - __clzll((long long)bits);
  }
  int next = -1;
  for (int b = p.nb - 1; b >= 0; --b) {
    const size_t o = base + (size_t)b * p.W;
    p.below[o] = next;
    const unsigned long long bits = p.bits[o];
    if (bits) next = b * BH + __ffsll((unsigned long long)bits) - 1;
  }
}

// g of row h0 + r of a (band, column): the nearest set bit at or below r, else the carry from above; likewise downwards
__device__ __forceinline__ unsigned g_of(unsigned long long bits, int r, int h0, int ab, int be) {
  const int h = h0 + r;
  const unsigned long long lo = bits & ((2ull << r) - 1ull), hi = bits >> r;
  const int up = lo ? h0 + 63 - __clzll((long long)lo) : ab;
  const int dn = hi ? h + __ffsll(hi) - 1 : be;
  unsigned g = SENT;
  if (up >= 0) g = (unsigned)(h - up);
  if (dn >= 0) g = min(g, (unsigned)(dn - h));
  return g;
}

// pixel (h, x) of image n, its squared distance and the column c the row pass found it in: the row of the target is the nearest
// set bit of column c at or above h, or the nearest below where that one is strictly nearer
__device__ __forceinline__ void near_store(const NearP& p, int n, int h, int x, int d2, int c) {
  const size_t pix = (size_t)h * p.W + x, o = (size_t)n * p.H * p.W + pix;
  if (p.max_dist2 > 0 && d2 > p.max_dist2) d2 = FAR_;
  int idx = -1;
  if (d2 != FAR_) {
    const int b = h / BH, h0 = b * BH, r = h - h0;
    const size_t t = ((size_t)n * p.nb + b) * p.W + c;
    const unsigned long long bits = p.bits[t];
    const unsigned long long lo = bits & ((2ull << r) - 1ull), hi = bits >> r;
    const int up = lo ? h0 + 63 - __clzll((long long)lo) : p.above[t];
    const int dn = hi ? h + __ffsll(hi) - 1 : p.below[t];
    idx = (up >= 0 && (dn < 0 || h - up <= dn - h) ? up : dn) * p.W + c;
  }
  if (p.dist2) p.dist2[o] = d2;
  if (p.index) p.index[o] = idx;
  const size_t s = idx >= 0 ? (size_t)idx : pix;                 // no target within the cap: the pixel's own word
  for (int i = 0; i < p.np; ++i) p.dst[i][o] = p.src[i][(size_t)n * p.ss[i] + s];
}

template <bool TRANSPOSED>
__global__ __launch_bounds__(256) void k_edt_cols(const EdtP p) {
  const int w = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y, n = blockIdx.z;
  if (w >= p.W) return;
  const size_t o = ((size_t)n * p.nb + b) * p.W + w;
  const unsigned long long bits = p.bits[o];
  const int ab = p.above[o], be = p.below[o], h0 = b * BH;
  if (TRANSPOSED) {
    // 64 values of one column are 128 contiguous, 128-byte aligned bytes of the transposed image (Hp is a multiple of 64)
    uint4* dst = reinterpret_cast<uint4*>(p.g + ((size_t)n * p.W + w) * p.Hp + h0);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      unsigned v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = g_of(bits, 8 * c + 2 * k, h0, ab, be) | (g_of(bits, 8 * c + 2 * k + 1, h0, ab, be) << 16);
      dst[c] = make_uint4(v[0], v[1], v[2], v[3]);
    }
  } else {
    unsigned short* dst = p.g + ((size_t)n * p.H + h0) * p.W + w;
    const int rows = min(BH, p.H - h0);
    for (int r = 0; r < rows; ++r) dst[(size_t)r * p.W] = (unsigned short)g_of(bits, r, h0, ab, be);
  }
}

template <class P>
__global__ __launch_bounds__(SEG) void k_edt_window(const P p) {
  constexpr bool IDX = std::is_same<P, NearP>::value;
  extern __shared__ int s2[];                  // [SEG + 2 R]
  const int tid = threadIdx.x, x0 = blockIdx.x * SEG, h = blockIdx.y, n = blockIdx.z, R = p.R;
  const unsigned short* g = p.g + ((size_t)n * p.H + h) * p.W;
  for (int k = tid; k < SEG + 2 * R; k += SEG) {
    const int x = x0 - R + k;
    int v = BIG2;
    if (x >= 0 && x < p.W) {
      const unsigned gv = g[x];
      if (gv != SENT) v = (int)(gv * gv);        // a column without a target is skipped, its sentinel never squared
    }
    s2[k] = v;
  }
  __syncthreads();
  const int x = x0 + tid;
  if (x >= p.W) return;
  int m = BIG2, jb = 0;
  for (int j = -R; j <= R; ++j) {
    const int v = j * j + s2[tid + R + j];
    if constexpr (IDX) {
      if (v < m) { m = v; jb = j; }              // left to right, replaced on < only: the smallest column among equals
    } else {
      m = min(m, v);
    }
  }
  // a candidate beyond the window contributes (R + 1)^2 or more: m is exact below that, and otherwise only known to lie above
  // the cap (< (R + 1)^2), where the distances are FAR and `within` is false anyway
  if constexpr (IDX) near_store(p, n, h, x, m > R * R + 2 * R ? FAR_ : m, x + jb);
  else edt_store(p, ((size_t)n * p.H + h) * p.W + x, m > R * R + 2 * R ? FAR_ : m);
}

__device__ __forceinline__ long long floordiv(long long a, long long b) {      // b > 0
  long long q = a / b;
  if ((a % b) < 0) --q;
  return q;
}

template <class P>
__global__ __launch_bounds__(64) void k_edt_envelope(const P p) {
  constexpr bool IDX = std::is_same<P, NearP>::value;
  const int h = blockIdx.x * 64 + threadIdx.x, n = blockIdx.y;
  if (h >= p.H) return;
  const int W = p.W;
  const size_t Hp = p.Hp, base = (size_t)n * W * Hp + h;
  const unsigned short* g = p.g + base;
  unsigned* stk = p.stk + base;
  int* out = p.d2t + base;
  int q = -1, sq = 0, tq = 0;
  long long gq2 = 0;
  for (int u = 0; u < W; ++u) {
    const unsigned gu = g[u * Hp];
    if (gu == SENT) continue;
    const long long gu2 = (long long)(gu * gu);
    while (q >= 0) {
      const long long ds = tq - sq, du = tq - u;
      if (ds * ds + gq2 <= du * du + gu2) break;
      if (--q >= 0) {
        const unsigned e = stk[q * Hp];
        sq = (int)(e & 0xFFFFu); tq = (int)(e >> 16);
        const unsigned gs = g[sq * Hp];
        gq2 = (long long)(gs * gs);
      }
    }
    if (q < 0) {
      q = 0; sq = u; tq = 0; gq2 = gu2;
    } else {
      // first abscissa from which parabola u lies at or below parabola sq: 64-bit, u^2 - sq^2 + g(u)^2 - g(sq)^2 passes 2^31
      const long long x = 1 + floordiv((long long)u * u - (long long)sq * sq + gu2 - gq2, 2ll * (u - sq));
      if (x < W) {
        stk[q * Hp] = ((unsigned)tq << 16) | (unsigned)sq;
        ++q; sq = u; tq = (int)x; gq2 = gu2;
      }
    }
  }
  if (q < 0) {                                   // a row of an image without a target
    for (int u = 0; u < W; ++u) out[u * Hp] = FAR_;
    return;
  }
  for (int u = W - 1; u >= 0; --u) {
    const long long d = u - sq;
    out[u * Hp] = (int)(d * d + gq2);
    if constexpr (IDX) p.colt[base + u * Hp] = (unsigned short)sq;
    if (u == tq && q > 0) {
      --q;
      const unsigned e = stk[q * Hp];
      sq = (int)(e & 0xFFFFu); tq = (int)(e >> 16);
      const unsigned gs = g[sq * Hp];
      gq2 = (long long)(gs * gs);
    }
  }
}

// d2t [W][Hp] -> the outputs [H][W] through a 64 x 65 LDS tile (64 x 64 values, a column of padding)
template <class P>
__global__ __launch_bounds__(256) void k_edt_transpose_out(const P p) {
  constexpr bool IDX = std::is_same<P, NearP>::value;
  __shared__ int tile[64][65];
  __shared__ unsigned short ctile[IDX ? 64 : 1][IDX ? 66 : 1];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6, n = blockIdx.z;
  const int x0 = blockIdx.x * 64, y0 = blockIdx.y * 64;
  const int* src = p.d2t + (size_t)n * p.W * p.Hp;
  for (int c = ty; c < 64; c += 4) {
    const int x = x0 + c, y = y0 + tx;
    if (x < p.W && y < p.H) {
      tile[c][tx] = src[(size_t)x * p.Hp + y];
      if constexpr (IDX) ctile[c][tx] = p.colt[((size_t)n * p.W + x) * p.Hp + y];
    }
  }
  __syncthreads();
  for (int r = ty; r < 64; r += 4) {
    const int y = y0 + r, x = x0 + tx;
    if (x < p.W && y < p.H) {
      if constexpr (IDX) near_store(p, n, y, x, tile[tx][r], ctile[tx][r]);
      else edt_store(p, ((size_t)n * p.H + y) * p.W + x, tile[tx][r]);
    }
  }
}

__global__ __launch_bounds__(256) void k_label_keep(const int* __restrict__ labels, const unsigned char* __restrict__ keep,
                                                    unsigned char* __restrict__ out, int M, size_t HW) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= HW) return;
  const size_t n = blockIdx.y;
  const int l = labels[n * HW + i];
  out[n * HW + i] = (l >= 0 && l <= M) ? keep[n * ((size_t)M + 1) + l] : 0;       // a value outside the table indexes nothing
}

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
bool edt_dims_ok(int N, int H, int W) {
  return N > 0 && H > 0 && W > 0 && N <= 65535 && H <= 32767 && W <= 32767 && (long long)H * W < (1ll << 31);
}
struct EdtLayout { size_t bits, above, below, g, stk, d2t, total; int nb, Hp; };
// the window pass needs the band tables and the row-major g only; the envelope the transposed g (rows padded to the band), its
// stack and its transposed result
EdtLayout edt_layout(int N, int H, int W, bool window) {
  EdtLayout l;
  l.nb = (H + BH - 1) / BH; l.Hp = l.nb * BH;
  const size_t tab = (size_t)N * l.nb * W, px = (size_t)N * W * l.Hp;
  size_t at = 0;
  l.bits = at; at += align256(tab * 8);
  l.above = at; at += align256(tab * 4);
  l.below = at; at += align256(tab * 4);
  l.g = at; at += align256(window ? (size_t)N * H * W * 2 : px * 2);
  l.stk = at; at += window ? 0 : align256(px * 4);
  l.d2t = at; at += window ? 0 : align256(px * 4);
  l.total = at;
  return l;
}
inline int isqrt_floor(int v) {
  int r = (int)sqrt((double)v);
  while ((long long)r * r > v) --r;
  while ((long long)(r + 1) * (r + 1) <= v) ++r;
  return r;
}

}  // namespace

extern "C" int sc_edt_variant(int H, int W, int max_dist2, int forced) {
  SC_REQUIRE(H > 0 && W > 0 && H <= 32767 && W <= 32767 && (long long)H * W < (1ll << 31),
             "sc_edt_variant: bad dims H=%d W=%d (1..32767, H*W < 2^31)", H, W);
  SC_REQUIRE(forced >= 0 && forced <= 2, "sc_edt_variant: forced=%d (0 the rule, 1 window, 2 envelope)", forced);
  const bool fits = max_dist2 > 0 && isqrt_floor(max_dist2) <= SC_EDT_WINDOW_MAX_R;
  SC_REQUIRE(forced != SC_EDT_WINDOW || fits, "sc_edt_variant: the window pass needs a cap with floor(sqrt(cap)) <= %d, got %d",
             SC_EDT_WINDOW_MAX_R, max_dist2);
  if (forced) return forced;
  return fits ? SC_EDT_WINDOW : SC_EDT_ENVELOPE;
}

extern "C" size_t sc_edt_workspace_bytes(int N, int H, int W) {
  if (!edt_dims_ok(N, H, W)) return 0;
  return edt_layout(N, H, W, false).total;
}

// the argument checks of a call and the row pass it takes (*cap: the cap that pass works under, -1 for none)
static int edt_plan(const sc_edt_args* a, int* variant_out, int* cap_out) {
  SC_REQUIRE(a && a->mask, "sc_edt: null pointer");
  const int N = a->N, H = a->H, W = a->W;
  SC_REQUIRE(edt_dims_ok(N, H, W), "sc_edt: bad dims N=%d H=%d W=%d (N <= 65535, H, W <= 32767, H*W < 2^31)", N, H, W);
  SC_REQUIRE(a->dist2 || a->dist || a->within, "sc_edt: no output requested");
  SC_REQUIRE(a->stride_n >= 0 && a->stride_h >= 0 && a->stride_w >= 0, "sc_edt: negative mask stride");
  SC_REQUIRE(a->max_dist2 >= 0 && a->thresh2 >= 0, "sc_edt: negative max_dist2 / thresh2");
  SC_REQUIRE(a->thresh2 < SC_EDT_FAR, "sc_edt: thresh2 must stay below SC_EDT_FAR (an image without a target is within nothing)");
  SC_REQUIRE(!a->dist || a->pixel_size > 0.0, "sc_edt: pixel_size must be positive");
  SC_REQUIRE(a->variant >= 0 && a->variant <= 2, "sc_edt: variant=%d (0 the rule, 1 window, 2 envelope)", a->variant);
  // the cap below which the result must be exact: max_dist2 for the distances, thresh2 for `within`
  const bool want_dist = a->dist2 || a->dist;
  int cap = -1;                                                    // none
  if (!want_dist) cap = a->thresh2;
  else if (a->max_dist2 > 0) cap = a->within && a->thresh2 > a->max_dist2 ? a->thresh2 : a->max_dist2;
  int variant;
  if (cap == 0) {                                                  // `within` at radius 0: a window of one pixel
    variant = a->variant ? a->variant : SC_EDT_WINDOW;
  } else {
    variant = sc_edt_variant(H, W, cap < 0 ? 0 : cap, a->variant);
    if (variant < 0) return variant;
  }
  *variant_out = variant; *cap_out = cap;
  return SC_OK;
}

extern "C" size_t sc_edt_call_workspace_bytes(const sc_edt_args* a) {
  int variant, cap;
  if (edt_plan(a, &variant, &cap) != SC_OK) return 0;
  return edt_layout(a->N, a->H, a->W, variant == SC_EDT_WINDOW).total;
}

extern "C" int sc_edt(const sc_edt_args* a, void* work, size_t work_bytes, sc_stream stream) {
  int variant, cap;
  const int rc = edt_plan(a, &variant, &cap);
  if (rc != SC_OK) return rc;
  SC_REQUIRE(work, "sc_edt: null pointer");
  SC_REQUIRE((reinterpret_cast<uintptr_t>(work) & 15) == 0, "sc_edt: the workspace must be 16-byte aligned");
  const int N = a->N, H = a->H, W = a->W;
  const bool want_dist = a->dist2 || a->dist;
  const EdtLayout l = edt_layout(N, H, W, variant == SC_EDT_WINDOW);
  SC_REQUIRE(work_bytes >= l.total, "sc_edt: workspace %zu < %zu bytes", work_bytes, l.total);
  hipStream_t st = (hipStream_t)stream;
  char* wk = static_cast<char*>(work);
  EdtP p{};
  p.mask = a->mask; p.sn = a->stride_n; p.sh = a->stride_h; p.sw = a->stride_w;
  p.N = N; p.H = H; p.W = W; p.invert = a->invert; p.nb = l.nb; p.Hp = l.Hp;
  p.bits = reinterpret_cast<unsigned long long*>(wk + l.bits);
  p.above = reinterpret_cast<int*>(wk + l.above); p.below = reinterpret_cast<int*>(wk + l.below);
  p.g = reinterpret_cast<unsigned short*>(wk + l.g);
  p.stk = reinterpret_cast<unsigned*>(wk + l.stk); p.d2t = reinterpret_cast<int*>(wk + l.d2t);
  p.max_dist2 = want_dist ? a->max_dist2 : 0; p.thresh2 = a->thresh2; p.negate = a->negate; p.pixel_size = a->pixel_size;
  p.dist2 = a->dist2; p.dist = a->dist; p.within = a->within;
  const dim3 cols((W + 255) / 256, l.nb, N);
  hipLaunchKernelGGL(k_edt_bits, cols, dim3(256), 0, st, p);
  SC_LAUNCH_OK("k_edt_bits");
  hipLaunchKernelGGL(k_edt_carry, dim3((W + 255) / 256, N), dim3(256), 0, st, p);
  SC_LAUNCH_OK("k_edt_carry");
  if (variant == SC_EDT_WINDOW) {
    p.R = isqrt_floor(cap);
    hipLaunchKernelGGL(k_edt_cols<false>, cols, dim3(256), 0, st, p);
    SC_LAUNCH_OK("k_edt_cols");
    hipLaunchKernelGGL(k_edt_window<EdtP>, dim3((W + SEG - 1) / SEG, H, N), dim3(SEG), (size_t)(SEG + 2 * p.R) * sizeof(int), st, p);
    SC_LAUNCH_OK("k_edt_window");
    return SC_OK;
  }
  hipLaunchKernelGGL(k_edt_cols<true>, cols, dim3(256), 0, st, p);
  SC_LAUNCH_OK("k_edt_cols");
  hipLaunchKernelGGL(k_edt_envelope<EdtP>, dim3((H + 63) / 64, N), dim3(64), 0, st, p);
  SC_LAUNCH_OK("k_edt_envelope");
  hipLaunchKernelGGL(k_edt_transpose_out<EdtP>, dim3((W + 63) / 64, (H + 63) / 64, N), dim3(256), 0, st, p);
  SC_LAUNCH_OK("k_edt_transpose_out");
  return SC_OK;
}

// sc_edt_nearest: the layout of sc_edt's row pass, then the envelope's transposed winning columns
static size_t near_total(const EdtLayout& l, int N, int W, bool window) {
  return l.total + (window ? 0 : align256((size_t)N * W * l.Hp * 2));
}

extern "C" size_t sc_edt_nearest_workspace_bytes(int N, int H, int W) {
  if (!edt_dims_ok(N, H, W)) return 0;
  return near_total(edt_layout(N, H, W, false), N, W, false);
}

static int near_plan(const sc_edt_nearest_args* a, int* variant_out) {
  SC_REQUIRE(a && a->mask, "sc_edt_nearest: null pointer");
  const int N = a->N, H = a->H, W = a->W;
  SC_REQUIRE(edt_dims_ok(N, H, W), "sc_edt_nearest: bad dims N=%d H=%d W=%d (N <= 65535, H, W <= 32767, H*W < 2^31)", N, H, W);
  SC_REQUIRE(a->n_planes >= 0 && a->n_planes <= SC_EDT_NEAREST_MAX_PLANES, "sc_edt_nearest: n_planes=%d (0..%d)", a->n_planes,
             SC_EDT_NEAREST_MAX_PLANES);
  SC_REQUIRE(a->index || a->dist2 || a->n_planes > 0, "sc_edt_nearest: no output requested");
  SC_REQUIRE(a->stride_n >= 0 && a->stride_h >= 0 && a->stride_w >= 0, "sc_edt_nearest: negative mask stride");
  SC_REQUIRE(a->max_dist2 >= 0, "sc_edt_nearest: negative max_dist2");
  SC_REQUIRE(a->variant >= 0 && a->variant <= 2, "sc_edt_nearest: variant=%d (0 the rule, 1 window, 2 envelope)", a->variant);
  for (int i = 0; i < a->n_planes; ++i) {
    SC_REQUIRE(a->src[i] && a->dst[i], "sc_edt_nearest: plane %d: null pointer", i);
    SC_REQUIRE(a->src[i] != a->dst[i], "sc_edt_nearest: plane %d: the destination must not be the source", i);
    SC_REQUIRE(a->src_stride[i] >= 0, "sc_edt_nearest: plane %d: negative source stride", i);
  }
  const int variant = sc_edt_variant(H, W, a->max_dist2, a->variant);
  if (variant < 0) return variant;
  *variant_out = variant;
  return SC_OK;
}

extern "C" size_t sc_edt_nearest_call_workspace_bytes(const sc_edt_nearest_args* a) {
  int variant;
  if (near_plan(a, &variant) != SC_OK) return 0;
  const bool window = variant == SC_EDT_WINDOW;
  return near_total(edt_layout(a->N, a->H, a->W, window), a->N, a->W, window);
}

extern "C" int sc_edt_nearest(const sc_edt_nearest_args* a, void* work, size_t work_bytes, sc_stream stream) {
  int variant;
  const int rc = near_plan(a, &variant);
  if (rc != SC_OK) return rc;
  SC_REQUIRE(work, "sc_edt_nearest: null pointer");
  SC_REQUIRE((reinterpret_cast<uintptr_t>(work) & 15) == 0, "sc_edt_nearest: the workspace must be 16-byte aligned");
  const int N = a->N, H = a->H, W = a->W;
  const bool window = variant == SC_EDT_WINDOW;
  const EdtLayout l = edt_layout(N, H, W, window);
  const size_t total = near_total(l, N, W, window);
  SC_REQUIRE(work_bytes >= total, "sc_edt_nearest: workspace %zu < %zu bytes", work_bytes, total);
  hipStream_t st = (hipStream_t)stream;
  char* wk = static_cast<char*>(work);
  NearP p{};
  p.mask = a->mask; p.sn = a->stride_n; p.sh = a->stride_h; p.sw = a->stride_w;
  p.N = N; p.H = H; p.W = W; p.invert = a->invert; p.nb = l.nb; p.Hp = l.Hp;
  p.bits = reinterpret_cast<unsigned long long*>(wk + l.bits);
  p.above = reinterpret_cast<int*>(wk + l.above); p.below = reinterpret_cast<int*>(wk + l.below);
  p.g = reinterpret_cast<unsigned short*>(wk + l.g);
  p.stk = reinterpret_cast<unsigned*>(wk + l.stk); p.d2t = reinterpret_cast<int*>(wk + l.d2t);
  p.colt = reinterpret_cast<unsigned short*>(wk + l.total);
  p.max_dist2 = a->max_dist2; p.pixel_size = 1.0;
  p.dist2 = a->dist2; p.index = a->index; p.np = a->n_planes;
  for (int i = 0; i < a->n_planes; ++i) {
    p.src[i] = static_cast<const unsigned*>(a->src[i]); p.ss[i] = a->src_stride[i]; p.dst[i] = static_cast<unsigned*>(a->dst[i]);
  }
  const EdtP& e = p;                                               // the column pass is sc_edt's own
  const dim3 cols((W + 255) / 256, l.nb, N);
  hipLaunchKernelGGL(k_edt_bits, cols, dim3(256), 0, st, e);
  SC_LAUNCH_OK("k_edt_bits");
  hipLaunchKernelGGL(k_edt_carry, dim3((W + 255) / 256, N), dim3(256), 0, st, e);
  SC_LAUNCH_OK("k_edt_carry");
  if (window) {
    p.R = isqrt_floor(a->max_dist2);
    hipLaunchKernelGGL(k_edt_cols<false>, cols, dim3(256), 0, st, e);
    SC_LAUNCH_OK("k_edt_cols");
    hipLaunchKernelGGL(k_edt_window<NearP>, dim3((W + SEG - 1) / SEG, H, N), dim3(SEG), (size_t)(SEG + 2 * p.R) * sizeof(int), st, p);
    SC_LAUNCH_OK("k_edt_window");
    return SC_OK;
  }
  hipLaunchKernelGGL(k_edt_cols<true>, cols, dim3(256), 0, st, e);
  SC_LAUNCH_OK("k_edt_cols");
  hipLaunchKernelGGL(k_edt_envelope<NearP>, dim3((H + 63) / 64, N), dim3(64), 0, st, p);
  SC_LAUNCH_OK("k_edt_envelope");
  hipLaunchKernelGGL(k_edt_transpose_out<NearP>, dim3((W + 63) / 64, (H + 63) / 64, N), dim3(256), 0, st, p);
  SC_LAUNCH_OK("k_edt_transpose_out");
  return SC_OK;
}

extern "C" int sc_label_keep(const int32_t* labels, const uint8_t* keep, uint8_t* out, int N, int M, int H, int W, sc_stream stream) {
  SC_REQUIRE(labels && keep && out, "sc_label_keep: null pointer");
  SC_REQUIRE(N > 0 && H > 0 && W > 0 && N <= 65535 && M >= 0 && (long long)H * W < (1ll << 31),
             "sc_label_keep: bad dims N=%d M=%d H=%d W=%d (N <= 65535, M >= 0, H*W < 2^31)", N, M, H, W);
  const size_t HW = (size_t)H * W;
  hipLaunchKernelGGL(k_label_keep, dim3((unsigned)((HW + 255) / 256), N), dim3(256), 0, (hipStream_t)stream, labels, keep, out, M, HW);
  SC_LAUNCH_OK("k_label_keep");
  return SC_OK;
}
