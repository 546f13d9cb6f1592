// Connected-component labelling and the plume label masks of starcop/data/mask_creation.py:6-27 (proposed_mask).
// One union-find engine, two front ends:
//   local   : one work-group per 64 x 64 tile.  proposed_mask stages T = mag1c >= threshold with a 3-pixel halo in LDS and
//             forms the erosion, the opening and the dilated opening D there; connected_components reads a ready mask.
//             Union-find inside the tile on an LDS parent array (atomicMin, the larger index always linked under the smaller),
//             then every set pixel gets the raster index (within its image) of its tile-local root; background gets -1.
//   merge   : one work-group per tile unions every set pixel of its right and bottom edges with its set neighbours across the
//             edge (with 8-connectivity the diagonals too, so a one-pixel diagonal through a tile corner joins).  Parents
//             only ever decrease; every read of a parent is an agent-scope atomic load and every write an agent-scope
//             atomicMin, because other work-groups (on other XCDs, each with its own L2) write the same array in this launch.
//   flatten : every set pixel resolves its root (the minimum raster index of its component, whatever order the atomics landed
//             in).  proposed_mask marks hit[root] for pixels with alpha != 0 (an int atomicOr into the flag byte's word) and
//             then writes T & D & hit[root]; connected_components ballots the roots into a bitmap, scans its popcounts per
//             image and numbers each component by the rank of its root in raster order (scipy.ndimage.label's numbering).
// Launches per call: 4 (proposed_mask) or 5 (connected_components), whatever the image holds; no host loop, no grid barrier,
// no work-group waits on another.
#include "sc_common.h"

namespace {

constexpr int TS = 64;                 // tile edge
constexpr int TP = TS * TS;            // pixels per tile
constexpr int HALO = 3;                // D depends on T within a radius-3 diamond (erosion, dilation, dilation)
constexpr int ST = TS + 2 * HALO;      // 70: staged T
constexpr int SE_ = TS + 4;            // 68: erosion
constexpr int SO = TS + 2;             // 66: opening

// flag byte per pixel (proposed_mask): bit 0 T, bit 1 D, bit 2 hit (set on a root by the flatten pass)
constexpr unsigned char F_T = 1, F_D = 2, F_HIT = 4;

__device__ __forceinline__ int lds_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ int g_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// path halving (atomicMin with the grandparent, an ancestor): without it a dense tile builds chains thousands deep
__device__ __forceinline__ int lds_find(int* s, int x) {
  int p = lds_load(s + x);
  while (p != x) {
    const int gp = lds_load(s + p);
    if (gp != p) atomicMin(s + x, gp);
    x = p; p = gp;
  }
  return x;
}
__device__ void lds_union(int* s, int a, int b) {
  for (;;) {
    a = lds_find(s, a); b = lds_find(s, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(s + a, b);
    if (old == a) return;
    a = old;                          // a was linked meanwhile: join its new parent with b
  }
}

// global parents of one image: P[i] <= i for a set pixel, -1 for background.  Path halving writes only ancestors (atomicMin),
// so the invariant holds whatever interleaving.
__device__ __forceinline__ int g_find(int* P, int x) {
  int p = g_load(P + x);
  while (p != x) {
    const int gp = g_load(P + p);
    if (gp != p) __hip_atomic_fetch_min(P + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = p; p = gp;
  }
  return x;
}
// read-only find for the flatten passes: every pixel of a tile passes through its tile root, so halving there would be 4096
// atomics on one address
__device__ __forceinline__ int g_find_ro(const int* P, int x) {
  int p = g_load(P + x);
  while (p != x) { x = p; p = g_load(P + x); }
  return x;
}
__device__ void g_union(int* P, int a, int b) {
  for (;;) {
    a = g_find(P, a); b = g_find(P, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(P + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == a) return;
    a = old;
  }
}

struct LabelP {
  // proposed_mask
  const float* mag; long long mag_stride;
  const unsigned char* alpha; long long alpha_stride;
  float thr; int se;
  unsigned char* flags;                // [N][H*W] (padded to whole words)
  unsigned char* out;                  // [N][H][W]
  // connected_components
  const unsigned char* mask; int conn8;
  unsigned long long* bits;            // [N][nw] root bitmap
  int* woff;                           // [N][nw] exclusive scan of the bitmap's popcounts
  int* counts;                         // [N]
  int* P;                              // [N][H*W] parents, then (connected_components) the labels
  int N, H, W, tx, nw;
};

// tile-local union-find on s[TP] (-1 = background, else the local index), then global parents out
__device__ void local_uf_and_store(const LabelP& p, int* s, int n, int x0, int y0, bool conn8) {
  const int tid = threadIdx.x;
  for (int i = tid; i < TP; i += 256) {
    if (lds_load(s + i) < 0) continue;              // the sign of an entry never changes: only the set ones are lowered
    const int r = i / TS, c = i % TS;
    const bool left = c > 0 && lds_load(s + i - 1) >= 0, up = r > 0 && lds_load(s + i - TS) >= 0;
    if (left) lds_union(s, i, i - 1);
    if (up) lds_union(s, i, i - TS);
    // 8-connectivity: with the pixel above set, both upper diagonals are its row neighbours (joined by their own left unions);
    // with the left pixel set, the upper-left one is its upper neighbour
    if (conn8 && r > 0 && !up) {
      if (c > 0 && !left && lds_load(s + i - TS - 1) >= 0) lds_union(s, i, i - TS - 1);
      if (c < TS - 1 && lds_load(s + i - TS + 1) >= 0) lds_union(s, i, i - TS + 1);
    }
  }
  __syncthreads();
  int* P = p.P + (size_t)n * p.H * p.W;
  for (int i = tid; i < TP; i += 256) {
    const int r = i / TS, c = i % TS, y = y0 + r, x = x0 + c;
    if (y >= p.H || x >= p.W) continue;
    int v = -1;
    if (lds_load(s + i) >= 0) {
      const int root = lds_find(s, i);
      v = (y0 + root / TS) * p.W + x0 + root % TS;
    }
    P[y * p.W + x] = v;
  }
}

// proposed_mask local pass: T, erosion, opening, D in LDS; union-find over D
__global__ __launch_bounds__(256) void k_pm_local(const LabelP p) {
  __shared__ unsigned char sT[ST * ST];
  __shared__ unsigned char sE[SE_ * SE_];
  __shared__ unsigned char sO[SO * SO];
  __shared__ int s[TP];
  const int tid = threadIdx.x, n = blockIdx.y;
  const int x0 = (blockIdx.x % p.tx) * TS, y0 = (blockIdx.x / p.tx) * TS;
  const int H = p.H, W = p.W, se = p.se;
  const float* mag = p.mag + (long long)n * p.mag_stride;
  // T outside the image is set: it never clears the erosion
  for (int i = tid; i < ST * ST; i += 256) {
    const int y = y0 - HALO + i / ST, x = x0 - HALO + i % ST;
    unsigned char t = 1;
    if (y >= 0 && y < H && x >= 0 && x < W) t = mag[(size_t)y * W + x] >= p.thr;      // NaN compares false
    sT[i] = t;
  }
  __syncthreads();
  if (se) {
    for (int i = tid; i < SE_ * SE_; i += 256) {
      const int ey = i / SE_, ex = i % SE_, y = y0 - 2 + ey, x = x0 - 2 + ex;
      unsigned char e = 0;
      if (y >= 0 && y < H && x >= 0 && x < W) {       // erosion outside the image is unset for the dilation that follows
        e = 1;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int c = 0; c < 3; ++c)
            if ((se >> (3 * r + c)) & 1) e &= sT[(ey + r) * ST + ex + c];
      }
      sE[i] = e;
    }
    __syncthreads();
    for (int i = tid; i < SO * SO; i += 256) {
      const int oy = i / SO, ox = i % SO, y = y0 - 1 + oy, x = x0 - 1 + ox;
      unsigned char o = 0;
      if (y >= 0 && y < H && x >= 0 && x < W) {
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int c = 0; c < 3; ++c)
            if ((se >> (3 * (2 - r) + (2 - c))) & 1) o |= sE[(oy + r) * SE_ + ox + c];
      }
      sO[i] = o;
    }
    __syncthreads();
  }
  unsigned char* fl = p.flags + (size_t)n * H * W;
  for (int i = tid; i < TP; i += 256) {
    const int r = i / TS, c = i % TS, y = y0 + r, x = x0 + c;
    const bool in = y < H && x < W;
    const unsigned char t = in ? sT[(r + HALO) * ST + c + HALO] : 0;
    unsigned char d = t;
    if (se) {
      d = 0;
#pragma unroll
      for (int rr = 0; rr < 3; ++rr)
#pragma unroll
        for (int cc = 0; cc < 3; ++cc)
          if ((se >> (3 * (2 - rr) + (2 - cc))) & 1) d |= sO[(r + rr) * SO + c + cc];
      d &= in ? 1 : 0;
    }
    s[i] = d ? i : -1;
    if (in) fl[(size_t)y * W + x] = (t ? F_T : 0) | (d ? F_D : 0);
  }
  __syncthreads();
  local_uf_and_store(p, s, n, x0, y0, true);
}

// connected_components local pass
__global__ __launch_bounds__(256) void k_cc_local(const LabelP p) {
  __shared__ int s[TP];
  const int tid = threadIdx.x, n = blockIdx.y;
  const int x0 = (blockIdx.x % p.tx) * TS, y0 = (blockIdx.x / p.tx) * TS;
  const unsigned char* m = p.mask + (size_t)n * p.H * p.W;
  for (int i = tid; i < TP; i += 256) {
    const int y = y0 + i / TS, x = x0 + i % TS;
    s[i] = (y < p.H && x < p.W && m[(size_t)y * p.W + x]) ? i : -1;
  }
  __syncthreads();
  local_uf_and_store(p, s, n, x0, y0, p.conn8 != 0);
}

// border merge: lanes 0..63 the tile's right edge, 64..127 its bottom edge.  Along one tile's edge, a pixel whose predecessor
// (same tile) is set inherits that lane's unions: the two are joined by the local pass, and so are neighbouring far-side pixels
// of one tile.  Every skipped pair is implied by the lane before it on the same edge and by pairs inside tiles, so the
// implications cannot form a cycle, and a run of set edge pixels inside one tile costs one union: the roots of a large
// component see few atomics.
__device__ __forceinline__ bool g_set(const int* P, int i) { return g_load(P + i) >= 0; }

__global__ __launch_bounds__(128) void k_merge(const LabelP p, int conn8) {
  const int n = blockIdx.y, H = p.H, W = p.W;
  const int x0 = (blockIdx.x % p.tx) * TS, y0 = (blockIdx.x / p.tx) * TS;
  int* P = p.P + (size_t)n * H * W;
  const int t = threadIdx.x & 63;
  const bool right = threadIdx.x < 64;
  // this lane's pixel a (near side) and the step along the edge (es) and across it (xs), as raster offsets
  const int y = right ? y0 + t : y0 + TS - 1, x = right ? x0 + TS - 1 : x0 + t;
  if (y >= H || x >= W) return;
  if (right ? x + 1 >= W : y + 1 >= H) return;
  const int along = right ? y : x, len = right ? H : W;
  const int es = right ? W : 1, xs = right ? 1 : W;
  const int a = y * W + x;
  if (!g_set(P, a)) return;
  const bool prev = t > 0 && g_set(P, a - es);               // the edge pixel before a, in this tile, is set
  const bool far0 = g_set(P, a + xs);                          // across the edge from a
  if (!conn8) {
    if (far0 && !(prev && g_set(P, a - es + xs))) g_union(P, a, a + xs);
    return;
  }
  const bool farp = along + 1 < len && g_set(P, a + es + xs);
  if (!prev) {
    if (along > 0 && g_set(P, a - es + xs)) g_union(P, a, a - es + xs);
    if (far0) g_union(P, a, a + xs);
  }
  if (farp && !(far0 && t < TS - 1)) g_union(P, a, a + es + xs);   // else a + es + xs joins a + xs inside the far tile
}

// proposed_mask flatten: P[i] = root; hit[root] |= alpha[i] != 0 (bit F_HIT of the root's flag byte, by a word atomicOr)
__global__ __launch_bounds__(256) void k_pm_hit(const LabelP p) {
  const int n = blockIdx.y;
  const int HW = p.H * p.W;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= HW) return;
  int* P = p.P + (size_t)n * HW;
  const int v = g_load(P + i);
  if (v < 0) return;
  const int r = g_find_ro(P, i);
  if (r != v) __hip_atomic_fetch_min(P + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (p.alpha[(long long)n * p.alpha_stride + i]) {
    const size_t b = (size_t)n * HW + r;
    unsigned* word = reinterpret_cast<unsigned*>(p.flags + (b & ~(size_t)3));
    __hip_atomic_fetch_or(word, (unsigned)F_HIT << (8 * (b & 3)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// proposed_mask output: T & D & hit[root]
__global__ __launch_bounds__(256) void k_pm_out(const LabelP p) {
  const int n = blockIdx.y;
  const int HW = p.H * p.W;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= HW) return;
  const size_t b = (size_t)n * HW;
  const unsigned char f = p.flags[b + i];
  unsigned char o = 0;
  if ((f & (F_T | F_D)) == (F_T | F_D)) o = (p.flags[b + p.P[b + i]] & F_HIT) ? 1 : 0;
  p.out[b + i] = o;
}

// connected_components flatten: one wave per 64 raster pixels; the roots (P[i] == i) of those pixels become one bitmap word
__global__ __launch_bounds__(256) void k_cc_roots(const LabelP p) {
  const int n = blockIdx.y;
  const int HW = p.H * p.W;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= p.nw) return;                // whole waves leave together
  const int i = w * 64 + (threadIdx.x & 63);
  int* P = p.P + (size_t)n * HW;
  bool root = false;
  if (i < HW) {
    const int v = g_load(P + i);
    if (v >= 0) {
      root = v == i;
      if (!root) {
        const int r = g_find_ro(P, i);
        if (r != v) __hip_atomic_fetch_min(P + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
  const unsigned long long m = __ballot(root);
  if ((threadIdx.x & 63) == 0) p.bits[(size_t)n * p.nw + w] = m;
}

// exclusive scan of the bitmap's popcounts, one work-group per image; counts[n] = the image's number of components
__global__ __launch_bounds__(256) void k_cc_scan(const LabelP p) {
  __shared__ int part[256];
  const int n = blockIdx.x, tid = threadIdx.x, nw = p.nw;
  const unsigned long long* bits = p.bits + (size_t)n * nw;
  int* woff = p.woff + (size_t)n * nw;
  const int per = (nw + 255) / 256, w0 = tid * per, w1 = min(nw, w0 + per);
  int sum = 0;
  for (int w = w0; w < w1; ++w) sum += __popcll(bits[w]);
  part[tid] = sum;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {   // Hillis-Steele inclusive scan
    const int v = tid >= o ? part[tid - o] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  int acc = part[tid] - sum;
  for (int w = w0; w < w1; ++w) { woff[w] = acc; acc += __popcll(bits[w]); }
  if (tid == 255) p.counts[n] = part[255];
}

// label = rank of the root among the image's roots in raster order + 1; background 0 (in place over the flattened parents)
__global__ __launch_bounds__(256) void k_cc_label(const LabelP p) {
  const int n = blockIdx.y;
  const int HW = p.H * p.W;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= HW) return;
  int* P = p.P + (size_t)n * HW;
  const int r = P[i];
  int lab = 0;
  if (r >= 0) {
    const size_t w = (size_t)n * p.nw + (r >> 6);
    lab = p.woff[w] + __popcll(p.bits[w] & ((1ull << (r & 63)) - 1ull)) + 1;
  }
  P[i] = lab;
}

inline int tiles_of(int H, int W) { return ((W + TS - 1) / TS) * ((H + TS - 1) / TS); }
inline int words_of(int H, int W) { return (int)(((long long)H * W + 63) / 64); }
inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
inline size_t pm_bytes(int N, int H, int W) {
  const size_t px = (size_t)N * H * W;
  return align256(px * 4) + align256((px + 3) & ~(size_t)3);
}
inline size_t cc_bytes(int N, int H, int W) {
  const size_t nw = (size_t)N * words_of(H, W);
  return align256(nw * 8) + align256(nw * 4);
}
bool dims_ok(int N, int H, int W) { return N > 0 && H > 0 && W > 0 && N <= 65535 && (long long)H * W < (1ll << 31); }

int merge(const LabelP& p, int conn8, hipStream_t st) {
  hipLaunchKernelGGL(k_merge, dim3(tiles_of(p.H, p.W), p.N), dim3(128), 0, st, p, conn8);
  SC_LAUNCH_OK("k_merge");
  return SC_OK;
}

}  // namespace

extern "C" size_t sc_label_workspace_bytes(int N, int H, int W) {
  if (!dims_ok(N, H, W)) return 0;
  const size_t a = pm_bytes(N, H, W), b = cc_bytes(N, H, W);
  return a > b ? a : b;
}

extern "C" int sc_connected_components(const uint8_t* mask, int connectivity, int32_t* labels, int32_t* counts, void* work,
                                       size_t work_bytes, int N, int H, int W, sc_stream stream) {
  SC_REQUIRE(mask && labels && counts && work, "sc_connected_components: null pointer");
  SC_REQUIRE(dims_ok(N, H, W), "sc_connected_components: bad dims N=%d H=%d W=%d (N <= 65535, H*W < 2^31)", N, H, W);
  SC_REQUIRE(connectivity == 1 || connectivity == 2, "sc_connected_components: connectivity=%d (1 or 2)", connectivity);
  SC_REQUIRE(work_bytes >= cc_bytes(N, H, W), "sc_connected_components: workspace %zu < %zu bytes", work_bytes, cc_bytes(N, H, W));
  hipStream_t st = (hipStream_t)stream;
  LabelP p{};
  p.mask = mask; p.conn8 = connectivity == 2; p.P = labels; p.counts = counts;
  p.N = N; p.H = H; p.W = W; p.tx = (W + TS - 1) / TS; p.nw = words_of(H, W);
  p.bits = reinterpret_cast<unsigned long long*>(work);
  p.woff = reinterpret_cast<int*>(static_cast<char*>(work) + align256((size_t)N * p.nw * 8));
  const int HW = H * W;
  hipLaunchKernelGGL(k_cc_local, dim3(tiles_of(H, W), N), dim3(256), 0, st, p);
  SC_LAUNCH_OK("k_cc_local");
  if (merge(p, p.conn8, st)) return SC_ERR_LAUNCH;
  hipLaunchKernelGGL(k_cc_roots, dim3((p.nw + 3) / 4, N), dim3(256), 0, st, p);
  SC_LAUNCH_OK("k_cc_roots");
  hipLaunchKernelGGL(k_cc_scan, dim3(N), dim3(256), 0, st, p);
  SC_LAUNCH_OK("k_cc_scan");
  hipLaunchKernelGGL(k_cc_label, dim3((HW + 255) / 256, N), dim3(256), 0, st, p);
  SC_LAUNCH_OK("k_cc_label");
  return SC_OK;
}

extern "C" int sc_proposed_mask(const float* mag1c, int64_t mag1c_plane_stride, const uint8_t* alpha, int64_t alpha_plane_stride,
                                float threshold, int se_bits, uint8_t* out, void* work, size_t work_bytes, int N, int H, int W,
                                sc_stream stream) {
  SC_REQUIRE(mag1c && alpha && out && work, "sc_proposed_mask: null pointer");
  SC_REQUIRE(dims_ok(N, H, W), "sc_proposed_mask: bad dims N=%d H=%d W=%d (N <= 65535, H*W < 2^31)", N, H, W);
  SC_REQUIRE(se_bits >= 0 && se_bits < 512, "sc_proposed_mask: se_bits=%d is not a 3x3 structuring element", se_bits);
  SC_REQUIRE(N == 1 || (mag1c_plane_stride >= (int64_t)H * W && alpha_plane_stride >= (int64_t)H * W),
             "sc_proposed_mask: plane strides %lld / %lld overlap %d x %d planes", (long long)mag1c_plane_stride,
             (long long)alpha_plane_stride, H, W);
  SC_REQUIRE(work_bytes >= pm_bytes(N, H, W), "sc_proposed_mask: workspace %zu < %zu bytes", work_bytes, pm_bytes(N, H, W));
  hipStream_t st = (hipStream_t)stream;
  LabelP p{};
  p.mag = mag1c; p.mag_stride = mag1c_plane_stride; p.alpha = alpha; p.alpha_stride = alpha_plane_stride;
  p.thr = threshold; p.se = se_bits; p.out = out;
  p.N = N; p.H = H; p.W = W; p.tx = (W + TS - 1) / TS;
  p.P = reinterpret_cast<int*>(work);
  p.flags = static_cast<unsigned char*>(work) + align256((size_t)N * H * W * 4);
  const int HW = H * W;
  hipLaunchKernelGGL(k_pm_local, dim3(tiles_of(H, W), N), dim3(256), 0, st, p);
  SC_LAUNCH_OK("k_pm_local");
  if (merge(p, 1, st)) return SC_ERR_LAUNCH;
  hipLaunchKernelGGL(k_pm_hit, dim3((HW + 255) / 256, N), dim3(256), 0, st, p);
  SC_LAUNCH_OK("k_pm_hit");
  hipLaunchKernelGGL(k_pm_out, dim3((HW + 255) / 256, N), dim3(256), 0, st, p);
  SC_LAUNCH_OK("k_pm_out");
  return SC_OK;
}
