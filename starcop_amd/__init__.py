"""starcop_amd: MI355X-native (gfx950) implementation of the STARCOP segmentation hot path.

Public surface (mirrors the reference):
  starcop_amd.model_module.ModelModule / configure_architecture / pred_classification / differences
  starcop_amd.model_setup.get_model
  starcop_amd.normalizer.DataNormalizer
  starcop_amd.padding.padded_predict / find_padding
  starcop_amd.mag1c.rmf / acrwl1mf / func_by_groups / generate_template_from_bands / get_mask_bad_bands
  starcop_amd.metrics
  starcop_amd.datamodule.ResidentTileSet / TrainLoader (HBM-resident training batches)
  starcop_amd.validation.run_validation ; starcop_amd.baselines.Mag1cBaseline / SanchezBaseline / VaronBaseline / binary_opening
  starcop_amd.features.FEATURES / extract_features / ratio_MLR_local (+ _5IN / _9IN / _5IN_simplediv) / mlr_fit /
    ratio_2c_match_c_from_sums_outlier / weight_mag1c
  starcop_amd.mask_creation.proposed_mask / connected_components / write_label_masks (the labelbinary target)
  starcop_amd.aviris.load_srf_wv3 / load_srf_s2 / transform_to_srf / transform_to_worldview_3 / transform_to_sentinel_2;
    starcop_amd.pipeline.aviris_as_sensor (the simulated WV3 / S2 bands of an AVIRIS-NG flight line);
    starcop_amd.resample.resize_antialiased / axis_taps / output_shape_for (those bands at the sensor's pixel size)
  starcop_amd.sampling.window_stats / stats_mag1c (mag1c statistics of every 512 x 512 window of a flight line) /
    mag1c_stats_dataframe / windows_intersect / select_non_overlapping / sampling_no_plumes (which windows become samples)
  starcop_amd.ortho.georeference / emit_geo_tags (orthorectification through a geometry look-up table); starcop_amd.mag1c.mag1c_emit
    (the EMIT driver with its georreferenced=True default); pipeline.emit_granule_predict(georeferenced=True, out_folder=...)
  starcop_amd.model_module_regression.ModelModuleRegression / l1 / mse (the regression twin; get_model serves both modes);
    starcop_amd.pointwise_net.SimpleCNN_v2 / SimpleCNN_v3; features.set_learned_model (the learned band-ratio product)
  starcop_amd.sentinel2.CDModel (predict / predict_scene: the whole-tile cloud mask) / scene_windows / cloud_mask_file / load_weights
  starcop_amd.scene.scene_windows / scene_table / table_rows / window_batches (the window plan of both predict_scene; sentinel2 re-exports it)
  starcop_amd.morphology.distance_transform / dilate / erode / opening / closing / remove_small_objects (exact Euclidean distance
    transform and disc morphology of masks); products.clean (opening, sieve and exclusion buffer of pred_binary; clean= on the
    scene calls); plumes.match_plumes(tolerance_px=...)
All compute runs in starcop_amd/libstarcop_hip.so (include/starcop_hip.h); there is no CPU fallback.
"""
__version__ = "0.1.0"
