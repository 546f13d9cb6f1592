"""Time of one reprojection (sc_warp / warp.reproject) next to a restatement with stock torch ops and to the numpy restatement, in
one process.

    python tools/bench_warp.py [--rounds 6] [--reps 10] [--out profiles/warp.txt]

Case: a seeded 2000 x 2300 geographic grid with an EMIT-like pixel (5.42e-4 degrees, ~60 m) warped onto the north-up UTM grid that
warp.suggest_grid gives at 60 m; five float32 planes (8 % no-data holes) and one uint8 mask.
  (a)  sc_warp: the library call alone (device events; output allocated once) -- five float32 planes nearest, the same bilinear,
       the uint8 mask nearest, and the coordinates-only call (P = 0, (u, v) written as float64), which shows how much of the time
       is the fp64 projection
  (b)  stock torch ops on the device: the same Krueger series as float64 tensor ops, index arithmetic, a gather and a where --
       coordinates recomputed in every call, as (a) does
  (c)  the numpy restatement of tests/warp_util.py, one run: a stated baseline, not a like-for-like comparison
(a) and (b) alternate in rounds of --reps calls after 3 warm-up calls each; the figure is the mean over all rounds, the spread the
minimum and maximum round.  Before anything is timed (a) and (b) are checked against (c): nearest bit-equal outside the pixels
within 1e-6 px of a cell boundary, bilinear within 2 * 2^-24 * max|x|.  Bytes: the output written once plus every source pixel
under the footprint read once, against the 4.25 / 4.70 TB/s of an access-pattern copy on this device.
"""
import argparse
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import warp_util as U  # noqa: E402
from starcop_amd import _lib, warp  # noqa: E402
from starcop_amd._lib import check, stream  # noqa: E402


def torch_clenshaw(c, xi, eta):
    s0, c0, sh0, ch0 = torch.sin(2 * xi), torch.cos(2 * xi), torch.sinh(2 * eta), torch.cosh(2 * eta)
    ar, ai = 2 * c0 * ch0, -2 * s0 * sh0
    y1r = y1i = y2r = y2i = torch.zeros_like(xi)
    for j in range(5, -1, -1):
        yr, yi = c[j] + ar * y1r - ai * y1i - y2r, ar * y1i + ai * y1r - y2i
        y2r, y2i, y1r, y1i = y1r, y1i, yr, yi
    zr, zi = s0 * ch0, c0 * sh0
    return zr * y1r - zi * y1i, zr * y1i + zi * y1r


def torch_taup(tau):
    t1 = torch.sqrt(1 + tau * tau)
    sig = torch.sinh(warp.E1 * torch.atanh(warp.E1 * tau / t1))
    return tau * torch.sqrt(1 + sig * sig) - sig * t1


def torch_source_coords(dst_shape, dst_gt, lon0, fn, inv, src_shape):
    """UTM destination over a geographic source with float64 tensor ops -> (u, v, inside)"""
    H, W = dst_shape
    col = torch.arange(W, dtype=torch.float64, device="cuda")[None, :] + 0.5
    row = torch.arange(H, dtype=torch.float64, device="cuda")[:, None] + 0.5
    e = dst_gt[0] + col * dst_gt[1] + row * dst_gt[2]
    n = dst_gt[3] + col * dst_gt[4] + row * dst_gt[5]
    xi, eta = (n - fn) / warp.KA, (e - 500000.0) / warp.KA
    dx, de = torch_clenshaw(warp.BETA, xi, eta)
    xip, etap = xi - dx, eta - de
    sx, cx, shp = torch.sin(xip), torch.cos(xip), torch.sinh(etap)
    taup = sx / torch.sqrt(shp * shp + cx * cx)
    lam = torch.atan2(shp, cx)
    tau = taup / warp.E2M
    for _ in range(warp.NEWTON_STEPS):
        ta = torch_taup(tau)
        tau = tau + (taup - ta) * (1 + warp.E2M * tau * tau) / (warp.E2M * torch.sqrt(1 + ta * ta) * torch.sqrt(1 + tau * tau))
    lon, lat = lon0 + torch.rad2deg(lam), torch.rad2deg(torch.atan(tau))
    u = inv[0] + lon * inv[1] + lat * inv[2]
    v = inv[3] + lon * inv[4] + lat * inv[5]
    inside = (lam.abs() <= math.radians(warp.MAX_DLON)) & (u >= 0) & (u < src_shape[1]) & (v >= 0) & (v < src_shape[0])
    return u, v, inside


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.require_device()
    lib = _lib.load()
    Hs, Ws, P, fill = 2000, 2300, 5, -9999.0
    px = 0.000542232520256367
    src_gt = (-104.03127, px, 0.0, 32.51731, 0.0, -px)
    dst_crs = warp.utm_crs_for(src_gt[0] + px * Ws / 2, src_gt[3] - px * Hs / 2)
    (H, W), dst_gt = warp.suggest_grid((Hs, Ws), src_gt, 4326, dst_crs, 60.0)
    inv = warp.invert_geotransform(src_gt)
    _, lon0, fnorth = warp.crs_kind(dst_crs)
    rng = np.random.default_rng(2000)
    src_np = (rng.standard_normal((P, Hs, Ws)) * 300 + 200).astype(np.float32)
    src_np[rng.random((P, Hs, Ws)) < 0.08] = fill
    mask_np = (rng.random((1, Hs, Ws)) < 0.3).astype(np.uint8)
    src, mask = torch.from_numpy(src_np).cuda(), torch.from_numpy(mask_np).cuda()
    out = torch.empty((P, H, W), dtype=torch.float32, device="cuda")
    out_mask = torch.empty((1, H, W), dtype=torch.uint8, device="cuda")
    coords = torch.empty((2, H, W), dtype=torch.float64, device="cuda")
    fill_bits = int(np.array(fill, dtype=np.float32).reshape(1).view(np.uint32)[0])

    def args_for(t, dst, mode, uv=None, planes=None):
        a = _lib.sc_warp_args()
        for i in range(6):
            a.dst_gt[i], a.src_inv[i] = dst_gt[i], inv[i]
        a.dst_crs, a.src_crs, a.out_h, a.out_w, a.src_h, a.src_w = dst_crs, 4326, H, W, Hs, Ws
        a.P = t.shape[0] if planes is None else planes
        a.elem_bytes, a.resampling = t.element_size(), mode
        for p in range(a.P):
            a.src[p] = t[p].data_ptr()
            a.row_stride[p], a.col_stride[p] = t.stride(1), t.stride(2)
            a.nodata_bits[p] = fill_bits if t.dtype == torch.float32 else 0
        a.out = dst.data_ptr() if a.P else None
        a.coords = uv.data_ptr() if uv is not None else None
        return a

    a_near, a_bil = args_for(src, out, _lib.WARP_NEAREST), args_for(src, out, _lib.WARP_BILINEAR)
    a_mask, a_uv = args_for(mask, out_mask, _lib.WARP_NEAREST), args_for(src, out, 0, coords, planes=0)
    fill_t = torch.tensor(fill, dtype=torch.float32, device="cuda")

    def run(a):
        return lambda: check(lib.sc_warp(a, stream()))

    def run_b():
        u, v, inside = torch_source_coords((H, W), dst_gt, lon0, fnorth, inv, (Hs, Ws))
        ix = torch.where(inside, torch.floor(u), torch.zeros_like(u)).long()
        iy = torch.where(inside, torch.floor(v), torch.zeros_like(v)).long()
        return torch.where(inside, src[:, iy, ix], fill_t), u, v, inside

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.reps          # ms per call

    # (c) first: the restatement is also what (a) and (b) are checked against before their times mean anything
    t = time.perf_counter()
    uv = U.source_coords_ref((H, W), dst_gt, dst_crs, src_gt, 4326, (Hs, Ws))
    want = U.nearest_ref(src_np, uv, [np.float32(fill)] * P)
    cpu = (time.perf_counter() - t) * 1e3
    keep = ~U.near_boundary(uv)
    assert (~keep).mean() <= 1e-3
    run(a_near)()
    assert U.mismatching_bytes(out.cpu().numpy()[:, keep], want[:, keep]) == 0, "sc_warp nearest disagrees with the numpy restatement"
    run(a_mask)()
    assert U.mismatching_bytes(out_mask.cpu().numpy()[:, keep], U.nearest_ref(mask_np, uv, [0])[:, keep]) == 0
    run(a_uv)()
    got_uv = coords.cpu().numpy()
    assert np.array_equal(np.isnan(got_uv), np.isnan(uv))
    err_uv = float(np.nanmax(np.abs(got_uv - uv)))
    assert err_uv <= 1e-6
    got_b, ub, vb, inside_b = run_b()
    assert np.array_equal(inside_b.cpu().numpy(), ~np.isnan(uv[0]))
    err_b = float(np.abs(torch.stack([ub, vb]).cpu().numpy() - uv)[:, ~np.isnan(uv[0])].max())
    assert err_b <= 1e-6 and U.mismatching_bytes(got_b.cpu().numpy()[:, keep], want[:, keep]) == 0, "torch restatement disagrees"
    del got_b, ub, vb, inside_b
    run(a_bil)()
    ref64, valid = U.bilinear_ref(src_np[0], uv, fill)
    got0 = out[0].cpu().numpy()
    gate = 2 * 2.0 ** -24 * float(np.abs(src_np[0][src_np[0] != fill]).max())
    m = keep & valid
    err_bil = float(np.abs(got0[m].astype(np.float64) - ref64[m].astype(np.float32).astype(np.float64)).max())
    assert err_bil <= gate and np.array_equal((got0.view(np.uint32) != fill_bits)[keep], valid[keep])

    fns = {"near": run(a_near), "bil": run(a_bil), "mask": run(a_mask), "uv": run(a_uv), "torch": run_b}
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            times[k].append(events(fn))
    mean = {k: float(np.mean(v)) for k, v in times.items()}

    def row(k):
        return f"{mean[k] * 1e3:9.1f} us per call   (rounds {min(times[k]) * 1e3:.1f} .. {max(times[k]) * 1e3:.1f})"
    inside = ~np.isnan(uv[0])
    touched = np.zeros((Hs, Ws), dtype=bool)
    touched[np.floor(uv[1][inside]).astype(np.int64), np.floor(uv[0][inside]).astype(np.int64)] = True
    moved = P * (H * W + int(touched.sum())) * 4
    lines = [
        f"warp, {Hs} x {Ws} geographic grid ({px:.6g} degrees) -> {H} x {W} EPSG:{dst_crs} grid at 60 m, {int(inside.sum())} of {H * W} pixels "
        f"inside the source ({100.0 * inside.mean():.1f} %), {P} float32 planes ({src_np.nbytes / 1e6:.1f} MB, 8 % no-data) and one uint8 mask; "
        f"{torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName})",
        f"{args.rounds} alternating rounds of {args.reps} calls after 3 warm-up calls each, device events; checked first against the numpy "
        f"restatement: nearest bit-equal ({int((~keep).sum())} pixels near a cell boundary left out), coordinates within {err_uv:.2g} px "
        f"(torch restatement {err_b:.2g} px), bilinear within {err_bil:.3g} (gate {gate:.3g})",
        f"(a) sc_warp nearest, {P} float32 planes, one launch   {row('near')}",
        f"(a) sc_warp bilinear, {P} float32 planes, one launch  {row('bil')}",
        f"(a) sc_warp nearest, the uint8 mask                  {row('mask')}",
        f"(a) sc_warp coordinates only (P = 0, float64 u, v)   {row('uv')}   = {100.0 * mean['uv'] / mean['near']:.0f} % of the nearest call",
        f"(b) stock torch ops (float64 series, index, where)   {row('torch')}   (b) / (a nearest) = {mean['torch'] / mean['near']:.1f}",
        f"(c) numpy restatement, coordinates + gather, one run {cpu:9.1f} ms   (c) / (a nearest) = {cpu / mean['near']:.0f}",
        f"bytes: {P} planes written ({P * H * W * 4 / 1e6:.1f} MB) + the {int(touched.sum())} source pixels under the footprint read once per plane "
        f"({P * int(touched.sum()) * 4 / 1e6:.1f} MB) = {moved / 1e6:.1f} MB -> (a nearest) {moved / (mean['near'] * 1e-3) / 1e12:.2f} TB/s, "
        f"{100.0 * moved / (mean['near'] * 1e-3) / 4.25e12:.0f} % / {100.0 * moved / (mean['near'] * 1e-3) / 4.70e12:.0f} % of the 4.25 / 4.70 TB/s "
        f"access-pattern copy; at that rate the bytes alone would take {moved / 4.25e12 * 1e6:.1f} us",
    ]
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
