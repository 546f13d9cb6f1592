// Device and host code shared by the operators that place destination pixels in source rasters: the warp (warp.hip, one source) and
// the mosaic (mosaic.hip, up to 64 sources).  WGS-84 Transverse Mercator as the Krueger series in the third flattening n to order
// n^6 (Karney 2011, "Transverse Mercator with an accuracy of a few nanometers", eq. 35 / 36), summed with a complex Clenshaw
// recurrence, the conformal latitude inverted with a FIXED number of Newton steps; and the sampling of one plane at (u, v): `nearest`
// copies element (floor(v), floor(u)) as a word, `bilinear` (float32) weighs the four pixels around (u - 0.5, v - 0.5) in fp64, leaves
// out samples that lie outside the raster, are NaN or carry the plane's no-data bit pattern, divides by the weight of those that
// count and rounds once.  Both operators include this file, so a pixel of one source gets the same arithmetic from either.  The
// footprint resampling (warp_area.hip) shares the projection and calls it on the host too, to estimate the size of a footprint.
// The host side of a grid pair lives here as well: its checks and route (grid_pair_setup), the point transform of a destination
// lattice point (grid_uv) and the plane descriptors (grid_planes) of sc_warp and sc_warp_area.
#pragma once
#include <math.h>

#include <cmath>

#include "sc_common.h"

namespace {

constexpr double WARP_DEG = 0.017453292519943295769;      // radians per degree
constexpr double WARP_MAX_DLON = 30.0;                    // degrees from the central meridian beyond which a point is outside
constexpr int WARP_NEWTON = 3;                            // steps of the conformal-latitude inversion: 2 reach the last place for |lat| < 89.999, one spare

struct Krueger {
  double e, e2m, ka;                             // first eccentricity, 1 - e^2, k0 * rectifying radius
  double alp[6], bet[6];
};

// sum_j c[j-1] sin(2 j (xi + i eta)), j = 1..6 -> (real, imaginary) part
__host__ __device__ __forceinline__ void clenshaw_sin(const double* c, double xi, double eta, double& re, double& im) {
  double s0, c0;
  sincos(2.0 * xi, &s0, &c0);
  const double sh0 = sinh(2.0 * eta), ch0 = cosh(2.0 * eta);
  const double ar = 2.0 * c0 * ch0, ai = -2.0 * s0 * sh0;              // 2 cos(2 zeta)
  double y1r = 0.0, y1i = 0.0, y2r = 0.0, y2i = 0.0;
#pragma unroll
  for (int j = 5; j >= 0; --j) {
    const double yr = c[j] + ar * y1r - ai * y1i - y2r;
    const double yi = ar * y1i + ai * y1r - y2i;
    y2r = y1r; y2i = y1i; y1r = yr; y1i = yi;
  }
  const double zr = s0 * ch0, zi = c0 * sh0;                           // sin(2 zeta)
  re = zr * y1r - zi * y1i;
  im = zr * y1i + zi * y1r;
}

// tangent of the conformal latitude from the tangent of the geographic one (Karney 2011 eq. 7-9)
__host__ __device__ __forceinline__ double taup_of(double tau, double e) {
  const double t1 = sqrt(1.0 + tau * tau);
  const double sig = sinh(e * atanh(e * tau / t1));
  return tau * sqrt(1.0 + sig * sig) - sig * t1;
}

// longitude / latitude in degrees -> easting / northing; false outside 30 degrees of the central meridian or |lat| > 90
__host__ __device__ __forceinline__ bool tm_forward(const Krueger& k, double lon0, double fn, double lon, double lat, double& E, double& N) {
  const double dl = remainder(lon - lon0, 360.0);
  if (!(fabs(dl) <= WARP_MAX_DLON) || !(fabs(lat) <= 90.0)) return false;
  const double taup = taup_of(tan(lat * WARP_DEG), k.e);
  double sl, cl;
  sincos(dl * WARP_DEG, &sl, &cl);
  const double xip = atan2(taup, cl), etap = asinh(sl / sqrt(taup * taup + cl * cl));
  double dx, de;
  clenshaw_sin(k.alp, xip, etap, dx, de);
  E = 500000.0 + k.ka * (etap + de);
  N = fn + k.ka * (xip + dx);
  return true;
}

// easting / northing -> longitude / latitude in degrees; false outside 30 degrees of the central meridian
__host__ __device__ __forceinline__ bool tm_inverse(const Krueger& k, double lon0, double fn, double E, double N, double& lon, double& lat) {
  const double xi = (N - fn) / k.ka, eta = (E - 500000.0) / k.ka;
  double dx, de;
  clenshaw_sin(k.bet, xi, eta, dx, de);
  const double xip = xi - dx, etap = eta - de;
  double sx, cx;
  sincos(xip, &sx, &cx);
  const double shp = sinh(etap);
  const double taup = sx / sqrt(shp * shp + cx * cx);
  const double lam = atan2(shp, cx);
  double tau = taup / k.e2m;
#pragma unroll
  for (int i = 0; i < WARP_NEWTON; ++i) {
    const double ta = taup_of(tau, k.e);
    tau += (taup - ta) * (1.0 + k.e2m * tau * tau) / (k.e2m * sqrt(1.0 + ta * ta) * sqrt(1.0 + tau * tau));
  }
  lat = atan(tau) / WARP_DEG;
  lon = lon0 + lam / WARP_DEG;
  return fabs(lam) <= WARP_MAX_DLON * WARP_DEG;
}

// a float32 sample takes part in an interpolation: not the plane's no-data pattern and not NaN
__device__ __forceinline__ bool counts(uint32_t bits, uint32_t nod) { return bits != nod && (bits & 0x7FFFFFFFu) <= 0x7F800000u; }

// the bilinear value of a float32 plane at (u, v) in fp64, BEFORE the rounding to float32.  The caller has established that the
// nearest pixel counts, so the weight sum is >= 0.25
__device__ __forceinline__ double bilinear_f64(const uint32_t* s, long long rs, long long cs, uint32_t nod, int sh, int sw, double u,
                                               double v) {
  const double ub = u - 0.5, vb = v - 0.5;
  const double fx0 = floor(ub), fy0 = floor(vb);
  const double fx = ub - fx0, fy = vb - fy0;
  const long long ix = (long long)fx0, iy = (long long)fy0;
  double acc = 0.0, wsum = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {                   // (row, column) offsets (0, 0), (0, 1), (1, 0), (1, 1)
    const long long xx = ix + (k & 1), yy = iy + (k >> 1);
    const double w = ((k & 1) ? fx : 1.0 - fx) * ((k >> 1) ? fy : 1.0 - fy);
    if (w > 0.0 && xx >= 0 && xx < sw && yy >= 0 && yy < sh) {
      const uint32_t b = s[yy * rs + xx * cs];
      if (counts(b, nod)) {
        acc += w * (double)__uint_as_float(b);
        wsum += w;
      }
    }
  }
  return acc / wsum;
}

// what a destination pixel gets from one plane at source coordinates (u, v): the plane's no-data when it is not inside; else the
// nearest element as a word, or (BIL: T = uint32_t, the bits of a float32) the bilinear value, no-data when the NEAREST element does
// not count.  (u, v) are only read when `inside`.
template <class T, bool BIL>
__device__ __forceinline__ T sample(const T* s, long long rs, long long cs, T nod, int sh, int sw, double u, double v, bool inside) {
  T val = nod;
  if (inside) val = s[(long long)floor(v) * rs + (long long)floor(u) * cs];
  if constexpr (BIL) {
    if (inside && counts(val, nod)) val = __float_as_uint((float)bilinear_f64(s, rs, cs, nod, sh, sw, u, v));
    else val = nod;
  }
  return val;
}

// 0 = affine only, 1 = WGS-84 geographic, 2 = WGS-84 UTM (zone and hemisphere set), -1 = not a code these operators know
inline int crs_kind(int code, double& lon0, double& fn) {
  lon0 = fn = 0.0;
  if (code == 4326) return 1;
  const bool north = code >= 32601 && code <= 32660, south = code >= 32701 && code <= 32760;
  if (!north && !south) return -1;
  lon0 = 6.0 * (code % 100) - 183.0;
  fn = south ? 10000000.0 : 0.0;
  return 2;
}

inline void krueger_wgs84(Krueger& k) {
  const double a = 6378137.0, f = 1.0 / 298.257223563, k0 = 0.9996;
  const double n = f / (2.0 - f), n2 = n * n, n3 = n2 * n, n4 = n3 * n, n5 = n4 * n, n6 = n5 * n;
  k.e = sqrt(f * (2.0 - f));
  k.e2m = (1.0 - f) * (1.0 - f);
  k.ka = k0 * a / (1.0 + n) * (1.0 + n2 / 4.0 + n4 / 64.0 + n6 / 256.0);
  k.alp[0] = n / 2 - 2 * n2 / 3 + 5 * n3 / 16 + 41 * n4 / 180 - 127 * n5 / 288 + 7891 * n6 / 37800;
  k.alp[1] = 13 * n2 / 48 - 3 * n3 / 5 + 557 * n4 / 1440 + 281 * n5 / 630 - 1983433 * n6 / 1935360;
  k.alp[2] = 61 * n3 / 240 - 103 * n4 / 140 + 15061 * n5 / 26880 + 167603 * n6 / 181440;
  k.alp[3] = 49561 * n4 / 161280 - 179 * n5 / 168 + 6601661 * n6 / 7257600;
  k.alp[4] = 34729 * n5 / 80640 - 3418889 * n6 / 1995840;
  k.alp[5] = 212378941 * n6 / 319334400;
  k.bet[0] = n / 2 - 2 * n2 / 3 + 37 * n3 / 96 - n4 / 360 - 81 * n5 / 512 + 96199 * n6 / 604800;
  k.bet[1] = n2 / 48 + n3 / 15 - 437 * n4 / 1440 + 46 * n5 / 105 - 1118711 * n6 / 3870720;
  k.bet[2] = 17 * n3 / 480 - 37 * n4 / 840 - 209 * n5 / 4480 + 5569 * n6 / 90720;
  k.bet[3] = 4397 * n4 / 161280 - 11 * n5 / 504 - 830251 * n6 / 7257600;
  k.bet[4] = 4583 * n5 / 161280 - 108847 * n6 / 3991680;
  k.bet[5] = 20648693 * n6 / 638668800;
}

// The grid pair of a kernel descriptor `d` (WarpD, AreaD: gt, inv, k, the four meridian fields, route) from the destination affine, the
// inverse source affine and the two CRS codes.  `who`: the entry point, for the messages.
template <class D>
int grid_pair_setup(D& d, const char* who, const double* dst_gt, const double* src_inv, int dst_crs, int src_crs) {
  for (int i = 0; i < 6; ++i) {
    SC_REQUIRE(std::isfinite(dst_gt[i]) && std::isfinite(src_inv[i]), "%s: geotransform term %d is not finite", who, i);
    d.gt[i] = dst_gt[i];
    d.inv[i] = src_inv[i];
  }
  SC_REQUIRE(dst_gt[1] * dst_gt[5] - dst_gt[2] * dst_gt[4] != 0.0, "%s: the destination geotransform is singular", who);
  SC_REQUIRE(src_inv[1] * src_inv[5] - src_inv[2] * src_inv[4] != 0.0, "%s: the inverse source geotransform is singular", who);
  d.route = 0;
  d.dst_lon0 = d.dst_fn = d.src_lon0 = d.src_fn = 0.0;
  if (dst_crs != src_crs) {                       // equal codes (0 included): affine only
    const int kd = crs_kind(dst_crs, d.dst_lon0, d.dst_fn), ks = crs_kind(src_crs, d.src_lon0, d.src_fn);
    SC_REQUIRE(kd > 0 && ks > 0, "%s: CRS pair %d -> %d (0 with 0, else 4326 or 32601..32660 / 32701..32760 on both sides)", who, dst_crs,
               src_crs);
    d.route = (kd == 2 ? 1 : 0) | (ks == 2 ? 2 : 0);   // bit 0: destination is UTM (inverse first), bit 1: source is UTM (forward after)
  } else {
    SC_REQUIRE(dst_crs >= 0, "%s: negative CRS code %d", who, dst_crs);
  }
  krueger_wgs84(d.k);
  return SC_OK;
}

// source pixel coordinates (u, v), unclipped, of the point (px, py) of the destination's pixel lattice: destination affine, the route
// through longitude / latitude, inverse source affine.  false when the projection cannot place the point
template <class D>
__host__ __device__ __forceinline__ bool grid_uv(const D& a, double px, double py, double& u, double& v) {
  double x = a.gt[0] + px * a.gt[1] + py * a.gt[2];
  double y = a.gt[3] + px * a.gt[4] + py * a.gt[5];
  bool ok = true;
  if (a.route & 1) ok = tm_inverse(a.k, a.dst_lon0, a.dst_fn, x, y, x, y);
  if (a.route & 2) ok = tm_forward(a.k, a.src_lon0, a.src_fn, x, y, x, y) && ok;
  u = a.inv[0] + x * a.inv[1] + y * a.inv[2];
  v = a.inv[3] + x * a.inv[4] + y * a.inv[5];
  return ok;
}

// The P source planes of a call `a` (sc_warp_args, sc_warp_area_args) into the descriptor `d` (src, rs, cs, nod), nothing beyond P
template <class D, class A>
int grid_planes(D& d, const char* who, const A* a, int eb) {
  for (int p = 0; p < SC_WARP_MAX_PLANES; ++p) {
    const bool on = p < a->P;
    if (on) SC_REQUIRE_PLANE(who, a->src[p], a->row_stride[p], a->col_stride[p], eb, p);
    d.src[p] = on ? a->src[p] : nullptr;
    d.rs[p] = on ? a->row_stride[p] : 0;
    d.cs[p] = on ? a->col_stride[p] : 0;
    d.nod[p] = on ? a->nodata_bits[p] : 0;
  }
  return SC_OK;
}

template <class T, int V>
struct alignas((V * sizeof(T) >= 16) ? 16 : V * sizeof(T)) Pack {
  T v[V];
};

}  // namespace
