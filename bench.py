"""bench.py -- 512x512 hyperspectral tiles/s of the HyperSTARCOP train step (fwd + loss + bwd + Adam).

    python bench.py --gpus N --steps K --warmup W [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

Workload (BASELINE.json configs[1]): the 4-channel (mag1c + RGB) MobileNetV2 U-Net, batch 16 per GPU, fp32,
synthetic seeded tiles resident in HBM, random-init weights.  A step is exactly ModelModule.training_step +
backward + Adam.step (reference model_module.py:69-88,172-185), executed by the HIP kernels with no autograd
graph.  One JSON line on rank 0; see DESIGN.md "Measurement" for the roofline / cpu_baseline definitions.

A plain run sets up, warms up, times the K steps and prints the line.  --full adds everything else, after the timed
region: the live roofline pass, the per-rank exchange diagnostics (N > 1), the fp32-x3 loop, `extra` and `cpu_baseline`
(--no-extras / --no-cpu-baseline leave out the last ones).  --dump-outputs DIR writes what the last timed step computed
(see dump_outputs) so that two builds can be compared output for output: the inputs and the initial weights are seeded.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

BF16_MFMA_PEAK_TFLOPS = 2500.0    # dense, MI355X_MICROARCH.md
HBM_PEAK_GBS = 8000.0
FP32_MFMA_PEAK_TFLOPS = 157.3      # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense


def synth_batch(B, H, W, seed, device):
    g = torch.Generator().manual_seed(seed)
    mag = (torch.randn(B, 1, H, W, generator=g) * 400).clamp(0, 10000)
    yy, xx = torch.meshgrid(torch.arange(H).float(), torch.arange(W).float(), indexing="ij")
    for b in range(0, B, 2):     # planted Gaussian-blob plume in half of the tiles
        cy, cx = float(torch.rand(1, generator=g)) * H, float(torch.rand(1, generator=g)) * W
        mag[b, 0] += 2000 * torch.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * 20.0 ** 2))
    ph = torch.rand(4, 3, generator=g) * 6.28
    rgb = torch.zeros(B, 3, H, W)
    for k in range(4):           # smooth field: sum of low-frequency cosines, spans the normaliser clip range
        rgb += torch.cos(yy[None, None] * (k + 1) * 6.28 / H + ph[k][None, :, None, None]) * torch.cos(xx[None, None] * (k + 1) * 6.28 / W)
    rgb = 57.5 + rgb * 13.0
    x = torch.cat([mag, rgb], 1).float()
    y = (mag > 500).float()
    w = (mag / 400).clamp(0.1, 1)
    return {"input": x.to(device), "output": y.to(device), "weight_loss": w.to(device)}


def cpu_baseline(budget_s=25.0):
    """The reference's CPU path (oracle restatement, torch CPU ops) timed on this box's host cores."""
    import torch.nn.functional as F
    from oracle.unet_ref import UnetMobileNetV2      # baseline leg only
    torch.manual_seed(0)
    B, H, W = 4, 512, 512
    net = UnetMobileNetV2(4, 1).train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    b = synth_batch(B, H, W, 99, "cpu")
    fac = torch.tensor([1750., 60., 60., 60.])[None, :, None, None]

    def step():
        logits = net(torch.clamp(b["input"] / fac, 0, 2))
        loss = (F.binary_cross_entropy_with_logits(logits, b["output"], reduction="none") * b["weight_loss"]).mean()
        opt.zero_grad(); loss.backward(); opt.step()

    step()                                            # warm-up
    t0 = time.perf_counter(); n = 0
    while True:
        step(); n += 1
        if time.perf_counter() - t0 > budget_s * 0.6 or n >= 8:
            break
    dt = time.perf_counter() - t0
    out = {"value": round(B * n / dt, 4), "unit": "tiles/s", "cores": torch.get_num_threads(), "kind": "port",
           "sample": f"{n} train steps of batch {B} x 4ch 512x512 fp32 (oracle/unet_ref.py + torch.optim.Adam) after 1 warm-up"}
    out["legs"] = cpu_baseline_legs(net, b, fac)
    return out


def cpu_baseline_legs(net, b, fac):
    """BASELINE.md section 3, legs B2-B4: the reference's CPU path (oracle restatements) for the workloads `extra` reports on the GPU
    -- eval forward / scene prediction, acrwl1mf per group (the reference's granularity) and batched, the two-band ratio -- each on a
    BOUNDED sample (a few seconds of host time), extrapolated to the unit of the matching `extra` entry."""
    import numpy as np
    from oracle import host_ref, mag1c_ref         # baseline legs only
    legs = {}
    cores = torch.get_num_threads()

    def wall(fn, min_reps=1, budget=3.0):
        fn()
        t0 = time.perf_counter(); n = 0
        while n < min_reps or (time.perf_counter() - t0 < budget and n < 20):
            fn(); n += 1
        return (time.perf_counter() - t0) / n, n
    # ---- B2: eval forward (4 tiles) and the notebook's padded_predict on a 1280 x 1242 scene (padding.py:13-50)
    net.eval()
    xin = torch.clamp(b["input"] / fac, 0, 2)
    with torch.no_grad():
        dt, n = wall(lambda: net(xin), budget=4.0)
        scene = np.random.default_rng(5).uniform(0, 2, size=(4, 1280, 1242)).astype(np.float32)
        dts, ns = wall(lambda: host_ref.padded_predict(scene, lambda a: torch.sigmoid(net(torch.from_numpy(a))).numpy()), budget=4.0)
    net.train()
    legs["B2_eval_forward"] = {"tiles_s": round(4 / dt, 3), "sample": f"{n} eval forwards of 4 x 4ch 512x512 (beside extra.infer_b16)", "cores": cores}
    legs["B2_predict_scene"] = {"ms": round(dts * 1e3, 1), "sample": f"{ns} padded_predict calls on a (4, 1280, 1242) scene (beside extra.predict_scene)", "cores": cores}
    # ---- B3: acrwl1mf, configs[2] shape (512-pixel column groups x 125 bands, float32, alpha 0, 30 iterations)
    g3 = np.load(os.path.join(ROOT, "tests", "golden", "g3_templates.npz"))
    rng = np.random.default_rng(7)
    S = 125
    t125 = np.interp(np.linspace(0, 72, S), np.arange(73), g3["aviris_template_kept"][:, 1])
    base = rng.uniform(1, 6, S)
    xg = (base * (1 + 0.05 * rng.standard_normal((64, 512, S)))).astype(np.float32)       # 64 of the tile's 512 column groups
    dt1, n1 = wall(lambda: [mag1c_ref.acrwl1mf_group(xg[i], t125.astype(np.float32)) for i in range(8)], budget=4.0)
    xt = torch.from_numpy(xg)
    dtb, nb = wall(lambda: mag1c_ref.acrwl1mf_batched(xt, t125), budget=4.0)
    legs["B3_mag1c_cfg3_per_group"] = {"tiles_s": round(1 / (dt1 / 8 * 512), 4), "sample": f"{n1} x 8 column groups of 512 px x 125 bands fp32, one call per group "
                                       "(mag1c.py:166-172 granularity; numpy / LAPACK), x 64 for the tile (beside extra.mag1c_cfg3)", "cores": cores}
    legs["B3_mag1c_cfg3_batched"] = {"tiles_s": round(1 / (dtb / 64 * 512), 4), "sample": f"{nb} calls on 64 groups at once ([b, P, S] torch CPU ops), x 8 for the tile", "cores": cores}
    # EMIT shape: 2560-pixel groups (1280 rows x column_step 2) x 49 bands, float64, alpha 1e-4
    te = g3["emit_template_kept"][:, 1]
    xe = (rng.uniform(1, 6, te.size) * (1 + 0.05 * rng.standard_normal((4, 2560, te.size)))).astype(np.float64)
    dte, ne = wall(lambda: [mag1c_ref.acrwl1mf_group(xe[i], te, alpha=1e-4) for i in range(4)], budget=4.0)
    legs["B3_mag1c_emit_per_group"] = {"ms_per_granule": round(dte / 4 * 621 * 1e3, 0), "sample": f"{ne} x 4 groups of 2560 px x {te.size} bands fp64, alpha 1e-4, x 621 / 4 for the "
                                       "granule (beside extra.mag1c_emit)", "cores": cores}
    # ---- B4: two-band ratio (feature_extration.py:42-56), numpy
    bg, sg = rng.uniform(0, 50, (512, 512)).astype(np.float32), rng.uniform(0, 50, (512, 512)).astype(np.float32)
    dtr, nr = wall(lambda: host_ref.band_ratio(bg, sg), min_reps=3, budget=2.0)
    legs["B4_band_ratio"] = {"tiles_s": round(1 / dtr, 2), "sample": f"{nr} calls on 2 x (512, 512) float32 (numpy percentiles; beside extra.band_ratio)", "cores": 1}
    return legs


CONV_ROOFLINE_TILES_S = 1718.0


def step_roofline(net, T, products):
    """Sum over the 63 convolutions x (forward, backward-data, backward-weight) of max(FLOP / P_layer, min bytes / 8 TB/s) per
    tile, with the ceilings the kernels here actually run on: the ten decoder 3x3 convolutions on the 16-bit matrix cores at
    2500 / `products` TFLOP/s fp32-equivalent (3 products: two fp16 terms; 6: three bf16 terms; 1: bf16), everything else (1x1,
    depthwise, stem, head) on the fp32 MFMA / VALU peak.  Min bytes = each pass reads its two operands / writes its result once
    (fp32; an upsampled source at its stored size).  Returns seconds per tile."""
    t = 0.0
    for op in net._ops:
        if op["type"] == "add":
            continue
        conv, o = op["conv"], op["out"]
        Ho = T >> o.shift
        macs = Ho * Ho * conv.out_channels * (conv.in_channels // conv.groups) * conv.kernel_size[0] ** 2
        elems = sum(t_.C * (T >> t_.shift) ** 2 for t_ in op["ins"]) + o.C * Ho * Ho
        peak = (BF16_MFMA_PEAK_TFLOPS / products if op["type"] == "conv3" else FP32_MFMA_PEAK_TFLOPS) * 1e12
        t += (2 if op["type"] == "stem" else 3) * max(2.0 * macs / peak, 4.0 * elems / (HBM_PEAK_GBS * 1e9))
    return t


def _timeit(fn, reps, best_of=1):
    """mean wall time of `reps` back-to-back calls after one warm-up call; best_of > 1: the fastest of that many such batches (the
    inference extras: single batches of 10 forwards showed sporadic one-off stalls of 10-30 ms on some boxes -- 3.05 / 6.12 / 3.09 ms per
    forward in three consecutive runs of this script -- that a per-call trace of the same sequence does not reproduce,
    tools/debug_eval_time.py)"""
    return _timeit_all(fn, reps, best_of)[0]


def _timeit_all(fn, reps, best_of=1):
    """(fastest, mean, median) over `best_of` batches of `reps` calls (the inference extras quote all three)"""
    fn(); torch.cuda.synchronize()
    dts = []
    for _ in range(best_of):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        dts.append((time.perf_counter() - t0) / reps)
    dts.sort()
    return dts[0], sum(dts) / len(dts), dts[len(dts) // 2]


def bench_extras(model, dev, precision):
    """The other BASELINE.json configurations, measured after the timed region (rank 0, N=1) so the driver sees them too:
    configs[2] mag1c on a 125-band AVIRIS-like tile, the EMIT-like granule of configs[4] (mag1c + scene inference), and the
    eval forward of the 4-channel U-Net.  Whole-call wall times with inputs resident in HBM; synthetic seeded data."""
    import numpy as np
    from starcop_amd import mag1c
    from starcop_amd import model_module as mm
    out = {}
    g3 = np.load(os.path.join(ROOT, "tests", "golden", "g3_templates.npz"))     # templates the reference generated (fixture: data)
    gen = torch.Generator(device=dev).manual_seed(7)

    def cube(H, W, templ):
        S = templ.size
        base = torch.rand(S, generator=gen, device=dev) * 5 + 1
        c = base * (1 + 0.05 * torch.randn(H, W, S, generator=gen, device=dev))
        conc = torch.zeros(H, W, device=dev); conc[H // 3:H // 3 + 60, W // 4:W // 4 + 40] = 2000.0
        return (c * (1 + conc[..., None] * 1e-5 * torch.as_tensor(templ, device=dev, dtype=torch.float32))).float().contiguous()

    # ---- configs[2]: AVIRIS-NG 125-band tile, one detector column per group (process_aviris.py:209-219), alpha = 0, 30 iterations
    S = 125
    t125 = np.interp(np.linspace(0, 72, S), np.arange(73), g3["aviris_template_kept"][:, 1])
    x = cube(512, 512, t125)
    groups = np.arange(1, 513)[None, :].repeat(512, 0)
    dt = _timeit(lambda: mag1c.acrwl1mf_by_groups(x, t125, groups), 5)
    dt0 = _timeit(lambda: mag1c.acrwl1mf_by_groups(x, t125, groups, num_iter=0), 5)
    # round 4: a group's radiances are loaded ONCE into the registers of its work-group (k_mag1c_tile<8, RES>); round 5: column groups
    # of <= 512 pixels take the DIRECT launch (no pack / scatter passes): HBM sees the cube TWICE -- the validity mask and the one tile
    # load -- plus the two float32 outputs; the 31 rounds run from registers and are bound by the fp64 VALU / the fp64 MFMA and their
    # barrier phases.  (VERDICT r5 #6a: the note priced the packed path's four passes until round 5.)
    hbm_bytes = (1 + 1) * 512 * 512 * S * 4 + 2 * 4 * 512 * 512
    it_flop = 31 * 2 * 2 * 512 * 512 * S                     # per-pixel dots + X^T w: two fp64 FMAs (and two f32 -> f64 conversions) per element and round
    out["mag1c_cfg3"] = {"workload": "configs[2]: 512x512 px x 125 bands fp32, 512 column groups, acrwl1mf num_iter=30 alpha=0",
                         "ms_per_tile": round(dt * 1e3, 3), "tiles_s": round(1 / dt, 1), "setup_ms": round(dt0 * 1e3, 3),
                         "roofline": {"bound": "latency of the per-group chain (fp64 VALU / fp64 MFMA phases between barriers; radiances resident in registers; "
                                               "HBM sees the cube twice: validity mask + the direct tile load -- nowhere near the HBM roof)",
                                      "hbm_frac": round(hbm_bytes / dt / 1e9 / HBM_PEAK_GBS, 4),
                                      "hbm_bytes_per_tile": hbm_bytes, "hbm_GBs": round(hbm_bytes / dt / 1e9, 1),
                                      "iteration_fp64_GFLOPs": round(it_flop / max(dt - dt0, 1e-9) / 1e9, 1), "fp64_vector_peak_GFLOPs": 78600.0,
                                      "iteration_frac_of_fp64_vector_peak": round(it_flop / max(dt - dt0, 1e-9) / 1e9 / 78600.0, 4),
                                      "note": "iteration time = ms_per_tile - setup_ms (setup: validity mask, layout, direct tile load, means, fp64-MFMA "
                                              "covariance, blocked Cholesky / inverse); every product needs a conversion too, so half of the issue slots at best"}}
    # ---- the same tile with ORTHORECTIFIED groups (process_aviris.py:211-217: |GLT sample index| varies along a row and down; 598
    # detector samples): the layout is a device counting sort (sc_mag1c_layout_ids) instead of torch sort / unique
    gl = ((np.arange(512)[None, :] + np.arange(512)[:, None] // 3) % 598 + 1).astype(np.int64)
    gl_d = torch.from_numpy(gl).to(dev)
    dtg = _timeit(lambda: mag1c.acrwl1mf_by_groups(x, t125, gl_d, max_group=598), 5)
    out["mag1c_glt"] = {"workload": "configs[2] tile with orthorectified (scattered) groups: 598 ids, ~438 px each, layout by device counting sort",
                        "ms_per_tile": round(dtg * 1e3, 3), "tiles_s": round(1 / dtg, 1)}
    # ---- EMIT-like granule (configs[4] preprocessing): 1280 x 1242 px, 49 bands in [2122, 2488] nm, fp64 arithmetic, alpha = 1e-4
    te = g3["emit_template_kept"][:, 1]
    raw = cube(1280, 1242, te)
    dt = _timeit(lambda: mag1c.mag1c_columns(raw, te, -9999.0, column_step=2), 3)
    # round 4 (k_mag1c_tile<4, ., SHRINK>): X is streamed ONCE per round (weights and X^T w in the same pass) + once for the means + five
    # covariance passes (two block pairs per pass at <= 64 bands) + mask and pack
    sw = (31 + 1 + 5 + 3) * 1280 * 1242 * te.size * 4
    out["mag1c_emit"] = {"workload": "EMIT-like 1280x1242 px x 49 bands fp32 storage / fp64 arithmetic, column_step=2 (621 groups), alpha=1e-4",
                         "ms_per_granule": round(dt * 1e3, 3), "Mpx_s": round(1280 * 1242 / dt / 1e6, 1),
                         "tile_equivalents_s": round(1280 * 1242 / 262144 / dt, 1),
                         "roofline": {"bound": "hbm", "streamed_bytes_per_granule": sw, "achieved_GBs": round(sw / dt / 1e9, 1), "peak_GBs": HBM_PEAK_GBS,
                                      "frac": round(sw / dt / 1e9 / HBM_PEAK_GBS, 3),
                                      "note": "X (float32) is streamed 40 times (round 3: 66); what keeps it from the HBM rate: the serial diagonal-block "
                                              "sweeps of the per-round factorisation of C_k (12 us of 42) and 621 groups on 256 CUs (three rounds, the "
                                              "third 43 % full); whole-call time incl. mask/layout/pack/scatter"}}
    # ---- two-band ratio on a batch of 512 x 512 tiles (feature_extration.py:42-56: exact 5 / 95 % trimmed sums + the ratio)
    from starcop_amd import features
    bg = torch.rand(16, 512, 512, generator=gen, device=dev) * 50
    sg = torch.rand(16, 512, 512, generator=gen, device=dev) * 50
    dtr = _timeit(lambda: features.ratio_2c_match_c_from_sums_outlier(bg, sg), 10)
    out["band_ratio"] = {"workload": "ratio_2c_match_c_from_sums_outlier on 16 x 2 x (512, 512) float32 tiles (exact radix-select percentiles)",
                         "tiles_s": round(16 / dtr, 1), "ms_per_16_tiles": round(dtr * 1e3, 3)}
    # ---- the path pytorch_lightning's Trainer.fit drives (scripts/train.py:140): training_step -> loss.backward() -> optimizer.step()
    # -> zero_grad(), i.e. the autograd Function + FusedAdam.step -- the timed region above is fused_train_step, asserted equal in results
    b16t = synth_batch(16, 512, 512, 1234, dev)
    opt_l = model.configure_optimizers()["optimizer"]

    def lightning_step():
        loss = model.training_step(b16t, 0)
        loss.backward()
        opt_l.step()
        opt_l.zero_grad()
    dtl = _timeit(lightning_step, 20)
    dtf = _timeit(lambda: model.fused_train_step(b16t, opt_l), 20)
    out["lightning_path"] = {"workload": "training_step + loss.backward() + optimizer.step() + zero_grad() at batch 16 (what Trainer.fit runs per batch)",
                             "tiles_s": round(16 / dtl, 1), "ms_per_step": round(dtl * 1e3, 3),
                             "fused_train_step_tiles_s_same_loop": round(16 / dtf, 1), "ratio_to_fused": round(dtf / dtl, 4)}
    # ---- U-Net inference
    model.eval()
    b16 = synth_batch(16, 512, 512, 77, dev)
    with torch.no_grad():
        dt, dt_mean, dt_med = _timeit_all(lambda: model(b16["input"]), 10, best_of=3)
        dtp = _timeit(lambda: model.batch_with_preds(b16), 10, best_of=3)
    out["infer_b16"] = {"workload": "eval forward, 16 x 4ch 512x512, precision " + precision + " (fastest of 3 batches of 10 forwards; mean / median beside it)",
                        "tiles_s": round(16 / dt, 1), "ms": round(dt * 1e3, 3),
                        "tiles_s_mean": round(16 / dt_mean, 1), "tiles_s_median": round(16 / dt_med, 1),
                        "batch_with_preds_tiles_s": round(16 / dtp, 1)}
    # round 6: inverted-residual blocks as one launch each in inference (csrc/conv_irb.hip) -- the same forward with them OFF, same process
    from starcop_amd import network as _nw
    plan16 = model.network._plans.get((16, 512, 512))
    out["infer_b16"]["fused_inverted_residual_blocks"] = len(getattr(plan16, "irb", {})) if plan16 is not None else None
    irb_saved, _nw._IRB = _nw._IRB, "0"
    model.network._plans.pop((16, 512, 512), None)
    with torch.no_grad():
        dt_sep = _timeit(lambda: model(b16["input"]), 10, best_of=3)
    _nw._IRB = irb_saved
    model.network._plans.pop((16, 512, 512), None)
    out["infer_b16"]["tiles_s_separate_launches"] = round(16 / dt_sep, 1)
    scene = np.random.default_rng(5).uniform(0, 100, size=(4, 1280, 1242)).astype(np.float32)
    dt = _timeit(lambda: model.predict(scene), 5)
    out["predict_scene"] = {"workload": "ModelModule.predict on a host (4, 1280, 1242) float32 scene: reflect-pad to x32, forward, sigmoid, crop, back to host",
                            "ms": round(dt * 1e3, 3), "Mpx_s": round(1280 * 1242 / dt / 1e6, 1)}
    # ---- configs[4] end to end on one GPU: EMIT-like cube -> mag1c (49 bands, fp64) -> RGB + rescale -> band ratio -> U-Net -> mask,
    # whole-scene forward and the tile-sharded form (512-row full-width strips + halo 320: what each rank of an N-GPU job runs on its share)
    from starcop_amd import pipeline
    wl = np.linspace(381.0, 2493.0, 285)
    keep = (wl >= 2122.0) & (wl <= 2488.0)
    te285 = np.interp(wl[keep], np.linspace(2122.0, 2488.0, te.size), te)
    gen2 = torch.Generator(device=dev).manual_seed(11)
    cube285 = (torch.rand(285, generator=gen2, device=dev) * 5 + 1) * (1 + 0.05 * torch.randn(1280, 1242, 285, generator=gen2, device=dev))
    cube285 = cube285.float().contiguous()
    dt_w = _timeit(lambda: pipeline.emit_scene_predict(model, cube285, wl, te285, column_step=2, ratio_bands=(2350, 2310)), 3)
    dt_t = _timeit(lambda: pipeline.emit_scene_predict(model, cube285, wl, te285, column_step=2, ratio_bands=(2350, 2310), tile=512), 3)
    out["emit_scene"] = {"workload": "configs[4]: EMIT-like 1280x1242x285 fp32 cube resident in HBM -> mag1c on the 49 bands in [2122, 2488] nm (fp64, column_step 2) "
                                     "-> RGB bands + range rescale -> two-band ratio -> U-Net eval forward -> probability + binary mask",
                         "ms_whole_scene_forward": round(dt_w * 1e3, 3), "ms_row_strips_512_halo_320": round(dt_t * 1e3, 3),
                         "scenes_s": round(1 / dt_w, 2), "tile_equivalents_s": round(1280 * 1242 / 262144 / dt_w, 1)}
    del cube285
    model.train()
    return out


DUMP_CAP = 7 << 20      # elements per dumped array (28 MiB as float32): the parameters (6.63 M) fit whole, the whole dump stays below 64 MB


def dump_outputs(out_dir, net, plan):
    """What a caller of the timed step receives from its last call, as float32 / float64 .npy files: the returned loss
    accumulator, the train-mode logits, the parameters after the Adam update and the BatchNorm running statistics.  An
    array above DUMP_CAP elements is stored as a fixed, seeded sample of its flattened elements (the same at every run)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    stats = [b.detach().reshape(-1) for b in net.buffers() if b.is_floating_point()]
    arrays = {"loss_sum": plan.loss_acc.detach().double(),                                 # sum of the weighted per-pixel losses
              "logits": plan.buf["logits"].detach().float(),
              "parameters": net.flat_parameters().detach().float(),
              "running_stats": torch.cat(stats).float() if stats else torch.zeros(0)}
    for i, (name, t) in enumerate(arrays.items()):
        a = t.cpu().numpy()
        if a.size > DUMP_CAP:
            idx = np.unique(np.random.default_rng(1000 + i).integers(0, a.size, DUMP_CAP))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(out_dir, name + ".npy"), a)


def self_launch(n, backend):
    """Re-executes this command line under torch.distributed.run with n ranks on this node (rendezvous on 127.0.0.1:free port)
    and returns its exit code.  The driver may call `python bench.py --gpus N` directly; every rank then runs main() with
    RANK / LOCAL_RANK / WORLD_SIZE set, exactly as under an external torchrun."""
    import socket
    import subprocess
    if backend == "nccl" and torch.cuda.device_count() < n:
        raise SystemExit(f"bench.py: --gpus {n} needs {n} visible GPUs, found {torch.cuda.device_count()} "
                         "(STARCOP_BENCH_BACKEND=gloo runs the N-rank path on fewer devices as a functional check only)")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")       # dmabuf IPC: required for RCCL between processes on this stack
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or n) // n)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100, help="timed steps (SURVEY 8d: >= 50)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=16, help="tiles per GPU (weak scaling)")
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--full", action="store_true", help="after the timed steps also run the live roofline pass, the per-rank exchange "
                    "diagnostics (N > 1), the fp32-x3 loop, `extra` and `cpu_baseline`; a plain run reports the timed steps only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the last timed step computed as DIR/<name>.npy "
                    "(loss, logits, updated parameters, BatchNorm running statistics; rank 0)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip `cpu_baseline`")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the fp32-x3 loop and the mag1c / inference measurements reported under `extra`")
    ap.add_argument("--overlap", type=int, default=1, help="1: weight gradients on a second HIP stream (default); 0: serial "
                    "launches (use for rocprofv3 per-kernel durations that match the roofline pass)")
    ap.add_argument("--precision", default="fp32", choices=["fp32", "fp32-x3", "fp32-bwd2", "fp32-2", "bf16"],
                    help="arithmetic of the >=32-channel 3x3 convolutions: fp32 (default, BASELINE configs[1], the parity mode: every fp32 operand split exactly "
                    "into two fp16 terms, three MFMA products) | fp32-x3 (three bf16 terms, six products: bit-faithful fp32 range) | fp32-bwd2 "
                    "(two bf16 terms in dgrad/wgrad) | fp32-2 (two bf16 terms everywhere) | bf16 (one term, configs[3]-style)")
    ap.add_argument("--gradsync", default=None, choices=["allreduce", "rs_ag"],
                    help="N > 1: gradient exchange of each bucket -- one all-reduce (default) or direct reduce-scatter + all-gather "
                         "on the same memory (SURVEY.md section 5; also STARCOP_GRADSYNC)")
    ap.add_argument("--graph", type=int, default=0, help="1: replay the step from a captured hipGraph (default: eager two-stream launches, measured faster)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    backend = os.environ.get("STARCOP_BENCH_BACKEND", "nccl")       # "gloo": functional check of the N>1 path on a 1-GPU box
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` with no rank environment: launch the N ranks ourselves (one process per GPU, RCCL)
        sys.exit(self_launch(args.gpus, backend))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}")
    if backend == "nccl" and torch.cuda.device_count() < world:
        raise SystemExit(f"bench.py: --gpus {world} needs {world} visible GPUs, found {torch.cuda.device_count()}")
    dev_index = local_rank if backend == "nccl" else local_rank % torch.cuda.device_count()
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    if world > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)            # nccl == RCCL over xGMI on ROCm
        else:
            dist.init_process_group(backend)
        world = dist.get_world_size()                                  # n_gpus / tile counts below come from the live process group

    from starcop_amd import model_module as mm
    from starcop_amd.parallel import GradSync
    torch.manual_seed(1234)                               # identical init on every rank
    model = mm.ModelModule(mm.default_settings(pos_weight=1, precision=args.precision)).to(dev).train()
    opt = model.configure_optimizers()["optimizer"]
    B, T = args.batch, args.tile
    batch = synth_batch(B, T, T, 1234 + rank, dev)
    sync = GradSync(world, mode=args.gradsync) if world > 1 else None
    net = model.network
    net.overlap_wgrad = bool(args.overlap)

    def step():
        return model.fused_train_step(batch, opt, grad_sync=sync)

    # ---- warm-up (also builds the plan); optionally capture the step into a hipGraph
    graph = None
    if world > 1:
        args.graph = 0        # RCCL collectives stay outside stream capture; eager launches are GPU-bound anyway
    n_eager = max(1, min(2, args.warmup)) if args.graph else args.warmup
    for _ in range(n_eager):
        step()
    torch.cuda.synchronize()
    if args.graph:
        try:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                step()
            torch.cuda.synchronize()
        except Exception as e:       # capture is an optimisation of launch overhead, never a correctness path
            if rank == 0:
                print(f"[bench] hipGraph capture unavailable ({type(e).__name__}: {e}); running eagerly", file=sys.stderr)
            graph = None
            torch.cuda.synchronize()
    run = (graph.replay if graph is not None else step)
    for _ in range(max(0, args.warmup - n_eager)):
        run()

    # ---- timed region
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        run()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    loss = float(net._plans[(B, T, T)].loss_acc.item()) / (B * T * T)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, net, net._plans[(B, T, T)])
    per_rank = None
    if world > 1:
        cdev = dev if backend == "nccl" else "cpu"
        own_ms = 1e3 * elapsed / args.steps
        t = torch.tensor([elapsed], device=cdev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if world > 1 and args.full:
        # ---- diagnostics of the exchange, OUTSIDE the timed region (every rank takes part): each rank's own step time and, from
        # device events around the two buckets of a few more steps, how much of the gradient exchange was NOT hidden behind the
        # encoder's backward -- what a first multi-GPU run needs to tell a slow rank from an exposed collective
        sync.timing = True
        acc, nd = [0.0, 0.0, 0.0], 5
        for _ in range(nd):
            step()
            tm = sync.collect_timing() or {}
            for i, k in enumerate(("overlap_window", "bucket_rest", "bucket_tail_wait")):
                acc[i] += tm.get(k, 0.0) / nd
        sync.timing = False
        mine = torch.tensor([own_ms] + acc, device=cdev, dtype=torch.float64)
        allr = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        per_rank = [{"rank": r, "ms_per_step": round(float(v[0]), 3), "overlap_window_ms": round(float(v[1]), 3),
                     "exposed_ms_bucket_encoder": round(float(v[2]), 3), "exposed_ms_bucket_decoder_wait": round(float(v[3]), 3)}
                    for r, v in enumerate(allr)]

    # ---- roofline of the dominant kernel family, measured live with events on the launch stream (eager, instrumented)
    roof = roof_streaming = roof_lowest = None
    if rank == 0 and args.full:
        net.profile = {}
        overlap, net.overlap_wgrad = net.overlap_wgrad, False     # serial launches: a kernel's events bracket only itself
        prof_steps = 3
        for _ in range(prof_steps):
            model.fused_train_step(batch, opt, grad_sync=None)     # rank-local: the other ranks are past the timed region
        torch.cuda.synchronize()
        prof = net.collect_profile()
        net.profile, net.overlap_wgrad = None, overlap
        tot_ms = sum(v["ms"] for v in prof.values())

        def roof_of(fam):
            d = prof[fam]
            ach = d["flop"] / (d["ms"] * 1e-3) / 1e12
            traffic, traffic_note = None, None
            bx3 = "bx3" in fam or "thin_h" in fam
            # k_conv3_bx3 / k_wgrad3_bx3 compute fp32-accurate products as 6 bf16 MFMAs: the ceiling for ALGORITHMIC flops is the
            # dense bf16 MFMA peak / 6; the fp32-MFMA kernels are priced against the fp32 matrix peak.
            tf_, tb_ = net._terms                                # bf16 terms per operand, forward / backward
            nterms = tb_ if ("dgrad)" in fam and "fwd" not in fam) or "wgrad" in fam else tf_
            nprod = {1: 1.0, 2: 3.0, 3: 6.0, 4: 3.0}[nterms]
            peak = BF16_MFMA_PEAK_TFLOPS / nprod if bx3 else FP32_MFMA_PEAK_TFLOPS
            # `traffic`: memory-side bytes per launch from rocprofv3 PMC passes.  Counters cannot be read from inside this process, so
            # the figure comes from the newest committed profile of this kernel family (profiles/r*_pmc_traffic_conv3_bx3.json, made by
            # tools/profile_round.sh -> tools/pmc_traffic.py from separate FETCH_SIZE / WRITE_SIZE passes over this same command) and
            # the note states its provenance.  Only the CALIBRATED figure is reported, and never one below the algorithmic bytes.
            if fam.startswith("k_conv3_bx3") and d.get("bytes"):
                import glob
                cands = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic_conv3_bx3.json")))
                alg = d["bytes"] / d["n"]
                for pmc in reversed(cands):
                    t = json.load(open(pmc))
                    if "hbm_bytes_per_launch_corrected" not in t:
                        continue
                    # per logical launch (one per layer and direction, the unit of `alg`): the step's bytes / this run's logical launches
                    # per step.  (Profiles without the per-step figure -- before r05f -- are per PHYSICAL launch: a data gradient cut
                    # into an up-sampled and a skip-channel launch counts twice there, which understated the ratio by 19-20 / 17.)
                    per_logical = (t["hbm_bytes_per_step_corrected"] / (d["n"] / max(prof_steps, 1))) if "hbm_bytes_per_step_corrected" in t else None
                    if per_logical is not None:
                        t = dict(t, hbm_bytes_per_launch_corrected=per_logical)
                    if t["hbm_bytes_per_launch_corrected"] < 0.98 * alg:
                        traffic_note = (f"{os.path.basename(pmc)} reports {t['hbm_bytes_per_launch_corrected'] / 1e6:.1f} MB per launch, below the "
                                        f"{alg / 1e6:.1f} MB algorithmic bytes of the launches timed here: refused (stale profile or a counter artefact)")
                        break
                    traffic = round(t["hbm_bytes_per_launch_corrected"])
                    traffic_note = (f"memory-side bytes per {'logical launch (the step total over this family / launches_per_step)' if per_logical is not None else 'physical launch'} "
                                    f"of {t['kernel_pattern']}* = {traffic / alg:.2f} x the algorithmic bytes; provenance: "
                                    f"profiles/{os.path.basename(pmc)} ({t.get('source', 'rocprofv3 --pmc')}; {t.get('launches', '?')} launches), FETCH_SIZE "
                                    f"(KiB -> bytes) divided by {t['fetch_calibration']['FETCH_SIZE_reported_over_known']:.3f} = what the counter reports of a KNOWN "
                                    "1 GiB stream in this kernel's 4 B/lane access pattern (profiles/r02_pmc_calibration.json), WRITE_SIZE calibrates to 1.000. "
                                    "Infinity-Cache hits are counted (MI355X_MICROARCH.md), so this is L2-miss traffic, an upper bound on HBM bytes. "
                                    "Not measured inside this run")
                    break
            hbm = ("<1>" in fam or "k_dw" in fam or "elementwise" in fam or "k_pw3_ebwd" in fam) and d.get("bytes")     # streaming families: HBM roofline
            if hbm:
                ach = d["bytes"] / (d["ms"] * 1e-3) / 1e9
                peak = HBM_PEAK_GBS
            exec_tf = None if hbm else nprod * d.get("flop_exec", d["flop"]) / (d["ms"] * 1e-3) / 1e12 if bx3 else ach
            return {"kernel": fam, "bound": "hbm" if hbm else "mfma", "achieved": round(ach, 2), "peak": round(peak, 1),
                    "unit": "GB/s" if hbm else "TFLOP/s",
                    "frac": round(ach / peak, 4),
                    #  like-for-like across rounds: the multiply-adds the matrix cores EXECUTE (sub-pixel layers: 16 of 36 taps; every
                    # product of the operand split counted) against the dense peak of the MFMA they run on -- `frac` above prices the
                    # reference's algorithmic FLOP against peak / products
                    "frac_executed": None if exec_tf is None else round(exec_tf / (BF16_MFMA_PEAK_TFLOPS if bx3 else FP32_MFMA_PEAK_TFLOPS), 4),
                    "executed_TFLOPs": None if exec_tf is None else round(exec_tf, 1),
                    "traffic": traffic, "traffic_note": traffic_note,
                    "peak_note": "HBM3E peak (MI355X_MICROARCH.md); achieved = algorithmic bytes of these launches / their time" if hbm else
                                 (f"fp32-equivalent ceiling of the {'two-fp16-term' if nterms == 4 else str(nterms) + '-bf16-term'} split: dense 16-bit MFMA peak "
                                  f"2500 TFLOP/s / {int(nprod)} products; `achieved` counts the ALGORITHMIC flops of the reference's 3x3 convolutions "
                                  f"(2 N H W Cout Cin 9); the kernels EXECUTE {round(nprod * d.get('flop_exec', d['flop']) / (d['ms'] * 1e-3) / 1e12, 1)} 16-bit TFLOP/s on the "
                                  f"matrix cores = {round(nprod * d.get('flop_exec', d['flop']) / (d['ms'] * 1e-3) / 1e12 / BF16_MFMA_PEAK_TFLOPS, 3)} of the dense 16-bit peak "
                                  f"({round(d.get('flop_exec', d['flop']) / d['flop'], 3)} of the algorithmic multiply-adds: the decoder conv1 layers run as sub-pixel "
                                  f"convolutions, 16 instead of 36 taps per low-resolution pixel and up-sampled channel, conv_sp.hip); "
                                  f"{round(ach / FP32_MFMA_PEAK_TFLOPS, 3)} x the fp32 MFMA peak of {FP32_MFMA_PEAK_TFLOPS}") if bx3 else
                                 "dense fp32 MFMA peak (v_mfma_f32_32x32x2_f32)",
                    "kernel_templates": ("k_conv3_bx3<Q,BNB,2,true>; launches with K loops of >= 16 chunks (decoder.blocks.0) run the "
                                         "wave-specialised k_conv3_ws<Q,BNB> of the same contraction; the decoder conv1 layers run as sub-pixel "
                                         "convolutions: k_conv3_sp<TW> (forward, decoder.blocks.0-3) and k_conv3_spd<TW> (data gradient of the "
                                         "up-sampled channels, decoder.blocks.0-2) -- all four names appear in the rocprofv3 kernel traces under "
                                         "profiles/.  decoder.blocks.4 (<= 16 output channels) is the thin-layer family (k_conv3_thin_h / "
                                         "k_conv3_thin_sp / k_conv3_thin_spd) -- since late round 6 including conv1's data gradient, which until then "
                                         "ran here as this family's slowest launch (153 TFLOP/s): the family is one launch per step smaller than in "
                                         "BENCH_r05 and its `frac` is not like-for-like with it (DESIGN 16 gives the like-for-like figure)") if (fam.startswith("k_conv3_bx3") and nterms == 4) else None,
                    "algorithmic_bytes_per_launch": round(d["bytes"] / d["n"]) if d.get("bytes") else None,
                    "algorithmic_flop_per_launch": round(d["flop"] / d["n"]),
                    "launches_per_step": d["n"] // prof_steps, "avg_launch_ms": round(d["ms"] / d["n"], 4),
                    "share_of_step_gpu_time": round(d["ms"] / tot_ms, 3),
                    "families_ms_per_step": {k: round(v["ms"] / 3, 3) for k, v in sorted(prof.items(), key=lambda kv: -kv[1]["ms"])}}

        # The dominant kernel = the family that carries most of the step's algorithmic FLOP (the 3x3 decoder convolutions: 88 % of
        # the network's MACs) -- stable from box to box, unlike "largest time", which flips between near-equal families.  The
        # largest HBM-priced (streaming) family by time is reported beside it.
        priced = [k for k in prof if prof[k]["flop"] or prof[k].get("bytes")] or list(prof)
        roof = roof_of(max(priced, key=lambda k: prof[k]["flop"]))
        streaming = [k for k in priced if ("<1>" in k or "k_dw" in k or "k_pw3_ebwd" in k) and prof[k].get("bytes")]
        roof_streaming = roof_of(max(streaming, key=lambda k: prof[k]["ms"])) if streaming else None
        if roof_streaming is not None:
            roof_streaming.pop("families_ms_per_step", None)
        # the family furthest below its own roof among those with >= 5 % of the step's GPU time (k_wgrad3_bx3)
        big = [k for k in priced if prof[k]["ms"] >= 0.05 * tot_ms and k != roof["kernel"]]
        roof_lowest = min((roof_of(k) for k in big), key=lambda r: r["frac"]) if big else None
        if roof_lowest is not None:
            roof_lowest.pop("families_ms_per_step", None)

    if rank == 0:
        tiles = world * B * args.steps
        out = {"metric": "512x512 hyperspectral tiles/sec (train fwd+bwd)", "value": round(tiles / elapsed, 2), "unit": "tiles/s",
               "n_gpus": dist.get_world_size() if world > 1 else 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(1e3 * elapsed / args.steps, 3),
               "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16" if args.precision == "bf16" else "f32", "data": "synthetic",
               "config": {"workload": "configs[1]: HyperSTARCOP U-Net (smp.Unet mobilenet_v2, 4ch mag1c+RGB) train step "
                                      "fwd+loss+bwd+Adam, 512x512 tiles, fp32 HIP kernels (3x3 convs: fp32 operands split exactly into 16-bit terms on the "
                                      "matrix cores, fp32 accumulation; see config.precision and DESIGN.md section 2)",
                          "batch_per_gpu": B, "global_batch": B * world, "tile": [4, T, T],
                          "parallelism": f"dp{world}", "hipgraph": graph is not None, "final_loss": round(loss, 6),
                          "precision": args.precision},
               "roofline": roof}
        if sync is not None:
            out["config"]["gradsync"] = sync.mode
        if per_rank is not None:
            out["per_rank"] = per_rank          # own (not max-over-ranks) step time; exposed = stream time the step waited for a bucket
        if roof_streaming is not None:
            out["roofline_streaming"] = roof_streaming
        if roof_lowest is not None:
            out["roofline_lowest"] = roof_lowest
        if T == 512 and args.precision != "bf16":
            # sum over the 63 conv layers of max(FLOP / fp32 peak, min bytes / HBM peak) = 0.582 ms per tile fwd+bwd
            out["conv_roofline"] = {"tiles_per_s_per_gpu": CONV_ROOFLINE_TILES_S,
                                    "frac": round(tiles / elapsed / world / CONV_ROOFLINE_TILES_S, 4),
                                    "note": "sum-of-layers fp32 conv roofline (157.3 TFLOP/s fp32 matrix peak, 8 TB/s HBM), 0.582 ms/tile"}
        if T == 512:
            nprod = {1: 1.0, 2: 3.0, 3: 6.0, 4: 3.0}[max(net._terms)]
            sr = step_roofline(net, T, nprod)
            out["step_roofline"] = {"tiles_per_s_per_gpu": round(1.0 / sr, 1), "ms_per_tile": round(sr * 1e3, 4),
                                    "frac": round(tiles / elapsed / world * sr, 4),
                                    "note": f"sum over layers x passes of max(FLOP / P, min bytes / 8 TB/s) with the ceilings these kernels run on: decoder 3x3 "
                                            f"convolutions 2500 / {int(nprod)} = {BF16_MFMA_PEAK_TFLOPS / nprod:.1f} TFLOP/s fp32-equivalent on the 16-bit MFMA, all other "
                                            f"layers {FP32_MFMA_PEAK_TFLOPS} TFLOP/s; the whole step (incl. loss, BatchNorm, Adam, which this floor prices at zero) "
                                            f"achieves {80.39 * tiles / elapsed / world / 1e3:.1f} TFLOP/s algorithmic"}
        if world == 1 and args.full and not args.no_extras:
            # the bit-faithful split (three bf16 terms, six products, fp32's exponent range) timed by the same loop
            if args.precision == "fp32" and T == 512:
                net.precision = "fp32-x3"
                for _ in range(3):
                    step()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                for _ in range(10):
                    step()
                torch.cuda.synchronize()
                out["config"]["precision_exact_tiles_s"] = round(B * 10 / (time.perf_counter() - t1), 2)
                net.precision = "fp32"
            out["extra"] = bench_extras(model, dev, args.precision)
        if args.full and not args.no_cpu_baseline and world == 1:       # reported at N=1 only (other ranks would idle at the exit barrier)
            out["cpu_baseline"] = cpu_baseline()
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
