"""Time of the feature transform (sc_edt_nearest / starcop_amd.morphology.nearest_index, expand_labels; plumes.background_rings)
next to the distance-only sc_edt call in the same process, to a restatement with stock torch ops and to scipy on the CPU.

    python tools/bench_nearest.py [--rounds 6] [--reps 10] [--out profiles/nearest.txt]

On the seeded 2000 x 2300 plume mask of tools/bench_component_stats.py (scene(..., seed=20002300)):
  (a) nearest_index unbounded (the envelope row pass) and at caps 3 / 16 / 64 (the window)
  (b) distance_transform(squared=True) at the same caps: (a) and (b) alternate, so (a) / (b) is the cost of the index over the
      distance alone, measured side by side
  (c) expand_labels(labels, 16) and background_rings(labels, 16, 2) on the connected_components labels of the mask
  (d) stock torch at cap 3 only: the minimum over the 29 shifted copies of the int64 key d2 * 2^32 + col * 2^16 + row
  (e) scipy distance_transform_edt(return_indices=True) on the CPU, one run
Rounds of ``reps`` calls after as many warm-up calls, device events; the figure is the mean over the rounds, the spread the
fastest and slowest round.  Everything is checked before it is timed: the unbounded index against scipy (the squared distance to
our index equals scipy's everywhere, the index is a target, and where the two indices differ -- ties -- ours has the smaller
(column, row)); window and envelope against each other at every cap; the cap-3 index against (d), which states the tie rule in
full; expand_labels and background_rings against a numpy gather through the checked index.
Bytes per call by index arithmetic: what sc_edt moves (tools/bench_morphology.py: edt_bytes), the index written, for the envelope
the transposed winning columns written and read, the band word and two carries of (band, winning column) as requested by every
pixel (16 bytes, scattered; neighbouring pixels mostly ask for the same ones), and 8 bytes per pixel and gathered plane."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from scipy import ndimage  # noqa: E402

from bench_component_stats import scene  # noqa: E402
from bench_morphology import alternate, edt_bytes, fmt, progress  # noqa: E402
from starcop_amd import _lib, mask_creation, morphology as mo, plumes  # noqa: E402

torch.set_num_threads(min(16, torch.get_num_threads()))
FAR = mo.FAR


def nearest_bytes(px, variant, index=True, dist2=False, planes=0):
    b = edt_bytes(px, variant, 4 if dist2 else 0)
    if variant == "envelope":
        b += px * (2 + 2)
    return b + px * (16 + (4 if index else 0) + 8 * planes)


def torch_nearest_cap3(target, H, W):
    """the restatement: min over the 29 offsets with dy^2 + dx^2 <= 9 of d2 * 2^32 + col * 2^16 + row of the shifted targets"""
    big = torch.iinfo(torch.int64).max
    pad = torch.nn.functional.pad(target, (3, 3, 3, 3))
    rows = torch.arange(H, device=target.device, dtype=torch.int64)[:, None]
    cols = torch.arange(W, device=target.device, dtype=torch.int64)[None, :]
    best = torch.full((H, W), big, dtype=torch.int64, device=target.device)
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            d2 = dy * dy + dx * dx
            if d2 > 9:
                continue
            key = (d2 << 32) + ((cols + dx) << 16) + (rows + dy)
            best = torch.minimum(best, torch.where(pad[3 + dy:3 + dy + H, 3 + dx:3 + dx + W], key, big))
    index = (best & 0xFFFF) * W + ((best >> 16) & 0xFFFF)
    return torch.where(best == big, -1, index).to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.require_device()
    H, W = 2000, 2300
    px = H * W
    mask = scene(H, W, 300, seed=20002300)[0].astype(np.uint8)
    d = torch.from_numpy(mask).cuda()
    lines = [f"feature transform; {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}); {H} x {W} plume mask, "
             f"{100.0 * mask.mean():.1f} % set; {args.rounds} alternating rounds of {args.reps} calls after {args.reps} warm-up calls each, "
             "device events; every result checked before it is timed; rates next to the 4.25 / 4.70 TB/s of the access-pattern copy "
             "(4- / 16-byte accesses)"]

    progress("scipy distance_transform_edt(return_indices=True)")
    t = time.perf_counter()
    sd, (sr, sc) = ndimage.distance_transform_edt(mask == 0, return_indices=True)
    cpu_ms = (time.perf_counter() - t) * 1e3
    sd2 = np.rint(sd ** 2).astype(np.int64)
    progress("unbounded index against scipy")
    gi, gd = mo.nearest_index(d, return_distance=True)
    index, d2 = gi.cpu().numpy().astype(np.int64), gd.cpu().numpy().astype(np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    r, c = index // W, index % W
    assert (index >= 0).all() and mask[r, c].all(), "an index that is no target"
    assert np.array_equal((yy - r) ** 2 + (xx - c) ** 2, sd2) and np.array_equal(d2, sd2), "not a nearest target"
    ties = (r != sr) | (c != sc)
    assert ((c < sc) | ((c == sc) & (r < sr)))[ties].all(), "a tie not broken towards the smaller (column, row)"
    lines.append(f"unbounded index: equal to scipy's on all but {int(ties.sum())} pixels ({100.0 * ties.mean():.2f} %), ties broken towards the "
                 "smaller (column, row) there")
    del yy, xx, sd, sr, sc
    rows = [("unbounded (envelope)", None, "envelope")]
    for cap in (3, 16, 64):
        progress(f"cap {cap}: window against envelope and the unbounded result")
        far = d2 > cap * cap
        wi = torch.from_numpy(np.where(far, -1, index).astype(np.int32)).cuda()
        wd = torch.from_numpy(np.where(far, FAR, d2).astype(np.int32)).cuda()
        for v in ("window", "envelope"):
            ci, cd = mo.nearest_index(d, max_distance=cap, return_distance=True, variant=v)
            assert torch.equal(ci, wi) and torch.equal(cd, wd), f"cap {cap}, {v}"
        assert torch.equal(mo.distance_transform(d, max_distance=cap, squared=True), wd)
        if cap == 3:
            progress("cap 3: the torch restatement against the index")
            assert torch.equal(torch_nearest_cap3(d != 0, H, W), wi), "the restatement disagrees at cap 3"
        rows.append((f"cap {cap} (window)", cap, "window"))
        del wi, wd
    labels, _ = mask_creation.connected_components(d)
    lab = labels.cpu().numpy()
    near = lab.reshape(-1)[index]
    progress("expand_labels and background_rings against the gather through the checked index")
    assert np.array_equal(mo.expand_labels(labels, 16).cpu().numpy(), np.where((lab == 0) & (d2 <= 256), near, lab))
    assert np.array_equal(plumes.background_rings(labels, 16, 2).cpu().numpy(), np.where((lab == 0) & (d2 > 4) & (d2 <= 256), near, 0))

    lines.append("(a) nearest_index (int32 index) | (b) distance_transform(squared=True), same cap | (a) / (b)")
    for label, cap, variant in rows:
        progress(f"timing {label}")
        fa = lambda cap=cap: mo.nearest_index(d, max_distance=cap)                             # noqa: E731
        fb = lambda cap=cap: mo.distance_transform(d, max_distance=cap, squared=True)          # noqa: E731
        ta, tb = alternate([fa, fb], args.rounds, args.reps)
        ba, bb = nearest_bytes(px, variant), edt_bytes(px, variant, 4)
        lines.append(f"{label:22s} (a) {fmt(ta)}  {ba / 1e6:.1f} MB -> {ba / (np.mean(ta) * 1e-3) / 1e12:.3f} TB/s   (b) {fmt(tb)}  {bb / 1e6:.1f} MB -> "
                     f"{bb / (np.mean(tb) * 1e-3) / 1e12:.3f} TB/s   (a) / (b) = {np.mean(ta) / np.mean(tb):.2f}")
        print(lines[-1], flush=True)
    progress("timing expand_labels and background_rings")
    te, tr = alternate([lambda: mo.expand_labels(labels, 16), lambda: plumes.background_rings(labels, 16, 2)], args.rounds, args.reps)
    be = nearest_bytes(px, "window", index=False, planes=1) + px * (4 + 1)                     # and the mask derived from the labels
    br = nearest_bytes(px, "window", index=False, dist2=True, planes=1) + px * (4 + 1) + px * 16  # and the select
    lines.append(f"(c) expand_labels(labels, 16)        {fmt(te)}  {be / 1e6:.1f} MB -> {be / (np.mean(te) * 1e-3) / 1e12:.3f} TB/s")
    lines.append(f"(c) background_rings(labels, 16, 2)  {fmt(tr)}  {br / 1e6:.1f} MB -> {br / (np.mean(tr) * 1e-3) / 1e12:.3f} TB/s")
    progress("timing the torch restatement at cap 3")
    target = d != 0
    ta, tt = alternate([lambda: mo.nearest_index(d, max_distance=3), lambda: torch_nearest_cap3(target, H, W)], args.rounds, args.reps)
    below = "every round of (a) below every round of (d)" if max(ta) < min(tt) else "NOT every round of (a) below every round of (d)"
    lines.append(f"cap 3: (a) {fmt(ta)}   (d) torch, 29 shifted keys {fmt(tt)}   (d) / (a) = {np.mean(tt) / np.mean(ta):.1f}: {below}")
    lines.append(f"(e) scipy distance_transform_edt(return_indices=True), one run on the CPU: {cpu_ms:.0f} ms")
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
