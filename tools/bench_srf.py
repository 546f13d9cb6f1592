"""Times of the simulated WV3 / S2 bands (sc_srf_bands) on a resident 4096 x 600 x 425 cube, of pipeline.aviris_as_sensor end to end
from a synthetic ENVI file (warm page cache), and of the numpy restatement per band for scale.

    python tools/bench_srf.py [--reps 20] [--e2e-lines 1024] [--tmp DIR]

Kernel rates are bytes of the band window [min band, max band] of the CSR (lines x samples x window x 4 B) per second, against the
6.29 TB/s float4 copy rate of MI355X HBM; device-event timing after warm-up, library call only.  The end-to-end rate is the file's
bytes per second of wall time (memmap -> pinned -> device -> kernel -> 34 deflate GeoTIFFs), against the 63 GB/s host link.
"""
import argparse
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import srf_util as U  # noqa: E402
from starcop_amd import aviris, pipeline  # noqa: E402

HBM = 6.29e12
HOST_LINK = 63e9


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps          # s per call


def csr(sensors, wl):
    ps, bs, ws = [np.zeros(1, np.int32)], [], []
    for sensor, (bands, srf) in U.all_sensor_weights().items():
        if sensor in sensors:
            p, b, w = aviris.srf_weights(bands, srf, wl)
            ps.append(p[1:] + ps[-1][-1]); bs.append(b); ws.append(w)
    return np.concatenate(ps), np.concatenate(bs), np.concatenate(ws)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--e2e-lines", type=int, default=1024)
    ap.add_argument("--tmp", default=None)
    args = ap.parse_args()
    wl = U.g3_grid()
    L, S, B = 4096, 600, wl.size
    rows = []
    g = torch.Generator(device="cuda").manual_seed(0)
    bip = torch.rand((L, S, B), generator=g, device="cuda") * 20.0
    for label, sensors in (("all 34 bands", ("WV3", "S2A", "S2B")), ("WV3 only (8)", ("WV3",))):
        p, b, w = csr(sensors, wl)
        plan = aviris.SrfPlan(p, b, w)
        nb = int(b.max() - b.min() + 1)
        out = torch.empty((plan.n_out, L, S), dtype=torch.float32, device="cuda")
        for layout in ("BIP", "BSQ"):
            x = bip if layout == "BIP" else bip.permute(2, 0, 1).contiguous().permute(1, 2, 0)
            t = timed(lambda: plan.run(x, out, -9999.0), args.reps)
            gbs = L * S * nb * 4 / t
            rows.append(("kernel", f"{layout}, {label}, window {nb} bands", t * 1e3, gbs / 1e9, gbs / HBM))
            del x
    del bip
    torch.cuda.empty_cache()

    # end to end from an ENVI file (BIP float32), warm page cache
    tmp = tempfile.mkdtemp(dir=args.tmp)
    try:
        ne = args.e2e_lines
        name = "ang20200101t000000_rdn_v2"
        folder = os.path.join(tmp, name)
        os.makedirs(folder)
        rng = np.random.default_rng(1)
        mm = np.lib.format.open_memmap(os.path.join(tmp, "scratch.npy"), mode="w+", dtype=np.float32, shape=(ne, S, B))
        for l0 in range(0, ne, 128):
            mm[l0:l0 + 128] = rng.uniform(0.0, 20.0, size=mm[l0:l0 + 128].shape).astype(np.float32)
        np.asarray(mm).tofile(os.path.join(folder, f"{name}_img"))
        del mm
        os.remove(os.path.join(tmp, "scratch.npy"))
        with open(os.path.join(folder, f"{name}_img.hdr"), "w") as f:
            f.write(f"ENVI\nsamples = {S}\nlines = {ne}\nbands = {B}\nheader offset = 0\ndata type = 4\ninterleave = bip\nbyte order = 0\n"
                    "map info = {UTM, 1, 1, 500000.0, 4100000.0, 5.0, 5.0, 11, North, WGS-84, units=Meters}\n"
                    f"wavelength units = Nanometers\nwavelength = {{ {', '.join(f'{v:.4f}' for v in wl)} }}\ndata ignore value = -9999\n")
        with open(os.path.join(folder, f"{name}_img"), "rb") as f:          # warm the page cache
            while f.read(1 << 26):
                pass
        aviris.SRF_WV3 = U.drop_zero_rows(U.wv3_table())
        aviris.SRF_S2 = U.drop_zero_rows(U.s2_table())
        nbytes = ne * S * B * 4
        for run in range(2):
            dst = os.path.join(tmp, f"out{run}")
            t0 = time.perf_counter()
            files = pipeline.aviris_as_sensor(folder, dst)
            t = time.perf_counter() - t0
            assert len(files) == 34
        rows.append(("aviris_as_sensor", f"{ne} x {S} x {B} BIP file -> 34 TIFFs", t * 1e3, nbytes / t / 1e9, nbytes / t / HOST_LINK))
        from starcop_amd import io_formats as io
        cube, _ = io.open_envi(os.path.join(folder, f"{name}_img"))
        sub = np.ascontiguousarray(cube[:64]).transpose(2, 0, 1)
        bands, srf = U.all_sensor_weights()["WV3"]
        t0 = time.perf_counter()
        U.oracle_transform(sub, bands, srf, wl, -9999.0)
        t = (time.perf_counter() - t0) / len(bands) * (L / 64)
        rows.append(("numpy restatement", f"per WV3 band, scaled from 64 to {L} lines of {S}", t * 1e3, float("nan"), float("nan")))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)

    print(f"{'what':20s} {'case':48s} {'ms':>10s} {'GB/s':>9s} {'of ceiling':>10s}")
    for what, case, ms, gbs, frac in rows:
        print(f"{what:20s} {case:48s} {ms:10.3f} {gbs:9.1f} {frac:10.1%}")


if __name__ == "__main__":
    main()
