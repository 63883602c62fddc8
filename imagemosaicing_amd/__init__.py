"""imagemosaicing_amd -- MI355X-native (gfx950, HIP) pairwise match + homography-warp hot path of
YuhuaXu/ImageMosaicing, behind the C ABI of include/mi355_mosaic.h.

This package is a thin ctypes binding of libmi355mosaic.so (hand-written HIP kernels + host C++).  It has
no CPU compute path: importing it needs the built library, creating a Context needs a gfx950 device.
The function names mirror the reference's own per-pair interface (Ransac2D, SelectMatchPairs,
ImageProjectionTransform, MosaicImagesRefined ...).
"""
from .capi import (  # noqa: F401
    Context, Mi355Error, lib_path, load_library, default_params, Params,
    SFPOINT, KEYPOINT, DMATCH, MATCHPAIR, PAIR_RESULT, CHIPINFO, IMAGE_TRANSFORM, FEATURE_HEADER, FEATURE_RECORD_BYTES, FEATURE_CHUNK_HEADER, FEATURE_CHUNK_ROWS, comm_unique_id, comm_available,
    mosaic_layout, blend_layout, pair_schedule, surf_pair_schedule, resample_by_overlap, write_match_pairs, load_match_pairs, write_match_pairs_txt,
    write_transforms, load_transforms, write_keypoints, load_keypoints, results_to_match_pairs, global_affine_align, select_connected,
    global_affine_align_results, select_connected_results, pair_moments_host, select_connected_moments, global_affine_align_moments, PAIR_MOMENTS, write_descriptors_xml, load_descriptors_xml,
    ScreenParams, screen_params, GainParams, GAIN_PAIR_STATS, gain_params, solve_gains,
    BlockGainParams, BLOCK_GAIN_STATS, block_gain_params, solve_block_gains,
    SharpParams, SHARP_PAIR_STATS, SHARP_FRAME_STATS, SHARP_KEPT, SHARP_DROPPED, SHARP_CUT_VERTEX, SHARP_NO_PAIR, sharp_params, solve_sharpness,
    select_sharp_frames, drop_sharp_frames,
    CoverParams, COVER_FRAME_STATS, COVER_BINS, COVER_NOT_CANDIDATE, COVER_DROPPED, COVER_KEPT_COVERAGE, COVER_CUT_VERTEX, COVER_NOT_EXAMINED,
    cover_params, cover_select,
    FeatherParams, feather_params, SeamlineParams, seamline_params, MedianParams, median_params, SeamCutParams, SeamReport, SEAM_CELL, seamcut_params, seam_grid, blend_seam_grid, seam_labels_host,
    Camera, UndistortParams, undistort_params, undistort_fit, undistort_map,
    PAIR_NORMAL_BLOCK, ProjectiveParams, ProjectiveReport, projective_params, pair_normal_blocks_host, global_projective_refine, global_projective_refine_results,
    PAIR_CALIB_BLOCK, CalibParams, CalibReport, calib_params, pair_calib_blocks_host, calibrate_lens, calibrate_lens_results, match_pairs_to_results,
    CALIB_K1, CALIB_K2, CALIB_P1, CALIB_P2, CALIB_K3,
    TieParams, tie_params, TIE_REPORT, TIE_NONE, TIE_REFINED, TIE_EDGE, TIE_FLAT, TIE_LOW, TIE_BORDER,
    TIE_FLAG_NOT_ACCEPTED, TIE_FLAG_NO_FRAME, TIE_FLAG_BAD_RECORD, TIE_FLAG_DEMOTED,
    LocalWarpParams, LOCAL_WARP_REPORT, local_warp_params, local_warp_stats_len, tie_residual_stats_host, solve_local_warps,
    VerifyParams, verify_params, PAIR_EDGE, PAIR_CYCLE, PAIR_RESIDUAL, VERIFY_REPORT, VERIFY_SUMMARY, EDGE_USABLE, EDGE_TESTABLE,
    VERDICT_NOT_USED, VERDICT_VERIFIED, VERDICT_ADMITTED, VERDICT_BRIDGE, VERDICT_REJECTED, VERDICT_UNDECIDED, VERIFY_SUSPECT,
    pair_edges_host, pair_cycles_host, pair_residuals_host, verify_pairs_results,
    GuidedParams, default_guided_params, guided_candidates, guided_candidates_count, merge_pair_results,
    PreviewParams, preview_params, overview_layout, NODATA_NONE, NODATA_ZERO, NODATA_MAP,
)

__all__ = [n for n in dir() if not n.startswith("_")]
