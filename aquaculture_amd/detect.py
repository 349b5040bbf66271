"""``yolov5/detect.py`` re-implemented on the HIP engine: same flags, same output files.

Reference call (reference README.md:77):

    python3 yolov5/detect.py --weights output/model_weights/multilabel_farms_exp2.pt \\
        --source data/jpegs --nosave --save-txt --save-conf

Output contract: ``<project>/<name>[N]/labels/<image stem>.txt``, one line per detection
``cls xc yc w h conf`` (``%g`` each, normalised by the original image size, ascending confidence), no file
for an image without detections -- consumed unchanged by reference src/process_yolo/geocode_results.py:123-172.

What differs from upstream's loop ([UPSTREAM detect.py run()]): images are decoded by a thread pool and run
through the engine in batches (``--batch-size``); with ``WORLD_SIZE > 1`` (torchrun) every rank takes the tiles
``i % world == rank`` and writes its own label files; detections are gathered over RCCL once at the end.
"""
from __future__ import annotations

import argparse
import os
import sys
import time
from pathlib import Path
from typing import List, Optional

import numpy as np
import torch

from . import dist as aqdist
from . import postprocess
from .checkpoint import load_checkpoint
from .dataloader import LoadImages, check_img_size, size_parts, split_decodable

UNSUPPORTED = ("view_img", "visualize", "update", "dnn")


def increment_path(path, exist_ok=False, sep="", mkdir=False) -> Path:
    """[UPSTREAM utils/general.py increment_path]: runs/detect/exp -> exp2, exp3, ..."""
    path = Path(path)
    if path.exists() and not exist_ok:
        for n in range(2, 9999):
            p = f"{path}{sep}{n}"
            if not os.path.exists(p):
                break
        path = Path(p)
    if mkdir:
        path.mkdir(parents=True, exist_ok=True)
    return path


def parse_opt(argv: Optional[List[str]] = None) -> argparse.Namespace:
    """Upstream's flag set plus --batch-size / --precision / --workers."""
    root = Path.cwd()
    p = argparse.ArgumentParser()
    p.add_argument("--weights", nargs="+", type=str, default="yolov5s.pt", help="model path")
    p.add_argument("--source", type=str, default="data/images", help="file/dir/glob")
    p.add_argument("--data", type=str, default="data/coco128.yaml", help="(unused: class names come from the checkpoint)")
    p.add_argument("--imgsz", "--img", "--img-size", nargs="+", type=int, default=[640], help="inference size h,w")
    p.add_argument("--conf-thres", type=float, default=0.25, help="confidence threshold")
    p.add_argument("--iou-thres", type=float, default=0.45, help="NMS IoU threshold")
    p.add_argument("--max-det", type=int, default=1000, help="maximum detections per image")
    p.add_argument("--device", default="", help="GPU ordinal (default: LOCAL_RANK or 0)")
    p.add_argument("--view-img", action="store_true")
    p.add_argument("--save-txt", action="store_true", help="save results to *.txt")
    p.add_argument("--save-conf", action="store_true", help="save confidences in --save-txt labels")
    p.add_argument("--save-crop", action="store_true",
                   help="save each detection's crop as <save_dir>/crops/<class>/<image stem>[k].jpg [UPSTREAM save_one_box]: pixels encoded on the GPU, "
                        "Huffman coding and files on host threads; byte-identical to Pillow's quality=95 4:4:4 JPEG of the same window")
    p.add_argument("--nosave", action="store_true",
                   help="do not write <save_dir>/<source file name>: every image with its detections drawn on it (boxes and labels drawn and the "
                        "JPEG's pixels encoded on the GPU; .jpg / .jpeg sources; quality 95, 4:2:0, as cv2.imwrite)")
    p.add_argument("--classes", nargs="+", type=int, help="filter by class: --classes 0, or --classes 0 2 3")
    p.add_argument("--agnostic-nms", action="store_true")
    p.add_argument("--augment", action="store_true",
                   help="augmented inference [UPSTREAM _forward_augment]: three passes (scale 1, 0.83 flipped left-right, 0.67), one NMS over all")
    p.add_argument("--visualize", action="store_true")
    p.add_argument("--update", action="store_true")
    p.add_argument("--project", default=str(root / "runs/detect"), help="save results to project/name")
    p.add_argument("--name", default="exp", help="save results to project/name")
    p.add_argument("--exist-ok", action="store_true", help="existing project/name ok, do not increment")
    p.add_argument("--line-thickness", default=3, type=int, help="bounding box thickness (pixels) in the saved images")
    p.add_argument("--hide-labels", default=False, action="store_true", help="no labels in the saved images")
    p.add_argument("--hide-conf", default=False, action="store_true", help="no confidences in the labels of the saved images")
    p.add_argument("--half", action="store_true", help="reduced precision (bf16 on MI355X; upstream: fp16)")
    p.add_argument("--dnn", action="store_true")
    p.add_argument("--vid-stride", type=int, default=1)
    p.add_argument("--batch-size", type=int, default=64, help="tiles per engine call")
    p.add_argument("--precision", choices=("fp32", "bf16", "fp8w", "f16x3", "fp8"), default=None,
                   help="default fp32 (detect.py without --half); fp8w = OCP e4m3 weights with per-channel power-of-two scales, bf16 activations")
    p.add_argument("--workers", type=int, default=8, help="jpeg decoders (worker processes for uniform tile directories, threads otherwise)")
    p.add_argument("--decode-threads", action="store_true", help="decode in threads of this process instead of worker processes")
    p.add_argument("--quiet", action="store_true", help="no per-image log line (the summary lines are still printed)")
    p.add_argument("--geocode-bboxes", default=None, metavar="CSV",
                   help="reference data/wanted_bboxes.csv: after the sweep, geocode every detection (the arithmetic of the "
                        "reference's src/process_yolo/geocode_results.py geocode_all_detections, as one batch op) -> --geocode-out")
    p.add_argument("--geocode-out", default=None, metavar="GEOJSON", help="default <save_dir>/detections.geojson")
    p.add_argument("--autotune", choices=("auto", "on", "off"), default="auto",
                   help="time the conv kernels' tile configurations on the first full batch and keep the fastest per layer "
                        "(cached in $AQ_TUNE_CACHE or ~/.cache/aquaculture_amd/); auto = only for sweeps of >= 8 batches per GPU")
    p.add_argument("--jpeg-decode", choices=("auto", "host", "split", "gpu"), default="auto",
                   help="split: the decode workers undo only the Huffman coding, the GPU does the inverse DCT, chroma upsampling and colour "
                        "conversion (byte-identical to libjpeg-turbo for every image inside the decoder's acceptance rule -- each block's IDCT "
                        "workspace within +-16383, three times what an encoder produces from 8-bit pixels; a file outside it, e.g. one with a "
                        "damaged quantisation table, ends the run with an error that names it; baseline 4:2:0 JPEGs, which is what the "
                        "reference's tiler writes); "
                        "host: full software decode in the workers; "
                        "gpu: the Huffman stage on the GPU as well (one lane per image, super-batches of AQ_JPEG_GPU_SUPERBATCH = 2048 tiles in "
                        "flight): the host only reads the files and strips byte stuffing, H2D carries the files' entropy-coded bytes; "
                        "auto: split when every image of the sweep qualifies, gpu when this rank's share is also >= AQ_JPEG_GPU_AUTO_MIN = "
                        "32768 images (measured on 65,536 1024-px tiles: gpu 10.4 k images/s steady and 0.84 s of start-up against split's 9.4 k "
                        "and 0.48 s -- 9.19 k vs 8.81 k over the whole sweep, break-even near 35 k images; same label bytes)")
    p.add_argument("--resume", action="store_true",
                   help="continue an interrupted sweep in project/name (implies --exist-ok): tiles recorded in the run directory's "
                        "done.rank*.txt manifests are skipped, also those that produced no label file")
    p.add_argument("--tile-scenes", nargs="?", type=int, const=1024, default=0, metavar="TILESIZE",
                   help="opt-in scene mode: --source holds whole scene rasters (*.tif); they are cut into TILESIZE (default 1024) tiles "
                        "on the GPU, in the order and with the names of reference src/load_data/tile_tifs.py, skipping its jpeg step")
    p.add_argument("--blank-key", nargs="?", const="", default=None, metavar="CSV",
                   help="also classify every image of the sweep as blank / partly blank / complete (the reference's is_blank and is_partly_blank, "
                        "src/utils.py:325-369) from the decoded pixels while they are on the GPU, and write the reference's "
                        "data/image_boxes_blank_key.csv (default <save_dir>/image_boxes_blank_key.csv) with the statistics as extra columns; "
                        "with --tile-scenes these are the raster's own pixels, not those of a JPEG round trip")
    p.add_argument("--blank-geom", nargs="?", const="", default=None, metavar="GEOJSON",
                   help="also outline the non-blank part of every partly blank image (the reference's correct_partly_blank_geom, src/utils.py:482-530: "
                        "the largest 8-connected region of max(R, G, B) < 250) on the GPU and write one polygon per such image (default "
                        "<save_dir>/image_boxes_partly_blank.geojson): in EPSG:3857 metres with --geocode-bboxes, else in pixels; implies --blank-key")
    p.add_argument("--blank-geom-simplify", type=float, default=0.5, metavar="TOL",
                   help="Douglas-Peucker tolerance in metres for the --blank-geom polygons in EPSG:3857 (the reference's simplify(0.5)); 0 disables it")
    p.add_argument("--facilities", nargs="?", const="", default=None, metavar="GEOJSON",
                   help="after the sweep and its geocoding, cluster the detections into candidate facilities (the reference's "
                        "src/process_yolo/calc_net_areas.py and src/cluster_facilities.py: per-cage area estimates, then DBSCAN of the cages' "
                        "EPSG:3035 centroids per year or image pass, on the GPU) and write them (default <save_dir>/facilities.geojson) with "
                        "their member detections beside them (<name>_detections.geojson); needs --geocode-bboxes")
    from .facilities import add_options as _facility_options
    _facility_options(p)
    p.add_argument("--land-filter", default=None, metavar="GEOJSON",
                   help="after the sweep and its geocoding, drop the detections whose boxes intersect the land polygons of GEOJSON (the reference's "
                        "remove_land_detections, src/process_yolo/geocode_results.py:200-218; its france_final_land_filter.shp as GeoJSON), the "
                        "box-against-polygon test on the GPU, and write what is left as the reference's ocean_detections.geojson; with "
                        "--facilities the ocean detections are clustered, as the reference does; needs --geocode-bboxes")
    p.add_argument("--ocean-out", default=None, metavar="GEOJSON", help="where --land-filter writes (default <save_dir>/ocean_detections.geojson)")
    from .land_images import add_options as _land_images_options
    _land_images_options(p)
    p.add_argument("--dedup-overlaps", nargs="?", const="", default=None, metavar="DIR",
                   help="right after the geocoding and before the land filter, count every cage once where the download boxes of the "
                        "--geocode-bboxes file overlap (the reference's deduplicate_download_boxes and deduplicate_gdf_with_bboxes, "
                        "src/utils.py:241-322: a box yields to every box before it in the file), the partner lists and the clip on the GPU; "
                        "writes dedup_detections.geojson, wanted_bboxes_dedup.geojson and dedup_overlaps.json (default <save_dir>); every "
                        "later step works on the survivors, and --evaluate, --evaluate-kfold and --model-errors pass their labels through "
                        "the same clip; detections.geojson stays as it is; needs --geocode-bboxes")
    p.add_argument("--evaluate", default=None, metavar="TRUTH_GEOJSON",
                   help="after the sweep, its geocoding, the land filter and the facilities, score the circle and square detections against the "
                        "human labels of TRUTH_GEOJSON (the reference's output/humanlabels.geojson) over the tuning grid of confidence threshold x "
                        "DBSCAN distance x minimum cluster size (the reference's src/get_kfold_cluster_performance.py), the neighbour search and "
                        "the box joins on the GPU, and write cluster_performance.csv and evaluation.json (the best rows, and the numbers at "
                        "--facilities-conf / -eps / -min-cages); with --land-filter the ocean detections are scored; needs --geocode-bboxes")
    from .evaluate import add_options as _evaluate_options
    _evaluate_options(p)
    p.add_argument("--model-errors", default=None, metavar="TRUTH_GEOJSON",
                   help="after the sweep, its geocoding and the land filter, join the circle and square detections of det_conf > "
                        "--model-errors-conf to the human labels of TRUTH_GEOJSON (the reference's output/humanlabels.geojson, with the labels' "
                        "pixel boxes and image sizes) -- each detection keeps the label of its year and type it overlaps most -- and fit one normal "
                        "to label area - detection area per image pass and cage type (the reference's define_model_error_distributions, "
                        "src/utils_tonnage.py:130-203), the join and the moments on the GPU; writes model_errors.csv, model_error_cages.csv and "
                        "model_errors.json, and --tonnage uses the table as its model errors; needs --geocode-bboxes, excludes --tonnage-errors")
    from .model_errors import add_options as _model_error_options
    _model_error_options(p)
    p.add_argument("--facility-sites", default=None, metavar="CSV",
                   help="directly after --facilities, on its facility table: which facilities lie within 1 km of a site the literature already "
                        "knew (CSV: lat, lon, num_cages; the reference's data/aquaculture_med_dedupe.csv) and which are additional production "
                        "locations, and how many distinct additional locations there are (the data behind the reference's "
                        "src/Results/FacilitiesMaps.py, without the plots), the facility rectangles and the box joins on the GPU; writes "
                        "facility_sites.geojson, facility_sites.csv and facility_sites.json; needs --facilities and --geocode-bboxes")
    from .facility_sites import add_options as _facility_sites_options
    _facility_sites_options(p)
    p.add_argument("--tonnage", nargs="?", const="", default=None, metavar="DIR",
                   help="after the sweep, its geocoding and the land filter, cluster the detections into facilities per image pass and estimate "
                        "their live-weight production per pass by the reference's bootstrap (src/utils_tonnage.py, "
                        "compute_facility_tonnage_estimates: K simulations of model error, area, depth, stocking density and harvest frequency), "
                        "simulated on the GPU, and write tonnage_estimates.csv, tonnage_facilities.csv and tonnage.json (default <save_dir>); "
                        "uses --facilities-conf / -eps / -min-cages; needs --geocode-bboxes and --tonnage-factors")
    from .tonnage import add_options as _tonnage_options
    _tonnage_options(p)
    from .bathymetry import add_options as _bathymetry_options
    _bathymetry_options(p)
    p.add_argument("--dedup-years", nargs="?", const="", default=None, metavar="DIR",
                   help="after the sweep, its geocoding and the land filter, keep one year's cages per tile and image pass (the reference's "
                        "dedup_cages_in_overlap_years_with_white_space, src/utils_tonnage.py:668-911: the years of a pass that cover the same tile "
                        "share its area in some order, each keeping its non-blank polygon minus the years before it), the pixel masks, the cages' "
                        "windows and the n! orders on the GPU; writes dedup_cages.csv, dedup_tiles.csv and dedup.json (default <save_dir>), and "
                        "--facilities (by pass), --bathymetry and --tonnage see the survivors only; needs --geocode-bboxes, implies --blank-geom")
    from .dedup import add_options as _dedup_options
    _dedup_options(p)
    p.add_argument("--performance", nargs="?", const="", default=None, metavar="DIR",
                   help="after the sweep and --evaluate, the numbers behind the reference's accuracy section (src/Results/ModelPerformance.py, "
                        "get_bucket_info_table, src/Results/upper_bound_calculation.R): precision and recall against the confidence threshold for "
                        "the raw detections, those outside the images wholly on land (--land-images) and those DBSCAN clusters once at "
                        "--performance-eps / -min-cages; the strata table with the labels extrapolated per stratum; and the Monte-Carlo upper "
                        "bound on the cage population, its Bernoulli samples drawn on the GPU; writes performance_curves.csv, "
                        "performance_strata.csv and performance.json (default <save_dir>); needs --evaluate and --geocode-bboxes")
    from .performance import add_options as _performance_options
    _performance_options(p)
    opt = p.parse_args(argv)
    if opt.dedup_years is not None and not opt.geocode_bboxes:
        p.error(DEDUP_NEEDS_GEOCODE)
    if opt.dedup_years is not None and opt.facilities is not None and opt.facilities_by != "pass":
        p.error(DEDUP_BY_PASS)
    if opt.dedup_years is not None and opt.blank_geom is None:
        opt.blank_geom = ""
    if opt.tonnage_missing is not None and (opt.tonnage is None or opt.dedup_years is None):
        p.error(MISSING_NEEDS_TONNAGE_DEDUP)
    if opt.tonnage_missing is not None:
        from .missing import parse_map
        try:
            parse_map(opt.tonnage_missing)
        except ValueError as e:
            p.error(str(e))
    if opt.tonnage_near_sites and opt.tonnage is None:
        p.error(NEAR_SITES_NEED_TONNAGE)
    if opt.bathymetry and not opt.geocode_bboxes:
        p.error("--bathymetry takes the depth under geocoded facilities: it needs --geocode-bboxes CSV (and --save-txt --save-conf)")
    if opt.bathymetry and opt.tonnage is None and opt.facilities is None:
        p.error("--bathymetry gives the facilities of --tonnage or --facilities their depth: it needs at least one of the two")
    if opt.bathymetry and opt.tonnage_depths:
        p.error("cage depths come from --bathymetry or from --tonnage-depths, not from both")
    if opt.tonnage is not None and not opt.geocode_bboxes:
        p.error("--tonnage estimates from geocoded detections: it needs --geocode-bboxes CSV (and --save-txt --save-conf)")
    if opt.tonnage is not None and not opt.tonnage_factors:
        p.error("--tonnage needs --tonnage-factors FILE (pass, s_mean, s_sd, h_mean, h_sd)")
    if opt.facilities is not None and not opt.geocode_bboxes:
        p.error("--facilities clusters geocoded detections: it needs --geocode-bboxes CSV (and --save-txt --save-conf)")
    if opt.land_filter is not None and not opt.geocode_bboxes:
        p.error("--land-filter filters geocoded detections: it needs --geocode-bboxes CSV (and --save-txt --save-conf)")
    if opt.land_images is not None and (opt.land_filter is None or not opt.geocode_bboxes):
        p.error(LAND_IMAGES_NEED_LAND)
    if opt.land_images is not None and opt.tile_scenes and not opt.evaluate_kfold_images:
        p.error(LAND_IMAGES_SCENES_NEED_IMAGES)
    if opt.land_images is not None and not (opt.land_images_indent > 0 and opt.land_images_indent < float("inf")):
        p.error(f"--land-images-indent {opt.land_images_indent}: a positive number of metres")
    if opt.dedup_overlaps is not None and not opt.geocode_bboxes:
        p.error(DEDUP_OVERLAPS_NEEDS_GEOCODE)
    if opt.evaluate is not None and not opt.geocode_bboxes:
        p.error("--evaluate scores geocoded detections: it needs --geocode-bboxes CSV (and --save-txt --save-conf)")
    if opt.model_errors is not None and not opt.geocode_bboxes:
        p.error(MODEL_ERRORS_NEED_GEOCODE)
    if opt.model_errors is not None and opt.tonnage_errors:
        p.error(MODEL_ERRORS_OR_FILE)
    if opt.facility_sites is not None and (opt.facilities is None or not opt.geocode_bboxes):
        p.error(FACILITY_SITES_NEED_FACILITIES)
    if opt.evaluate_kfold is not None and opt.evaluate is None:
        p.error(KFOLD_NEEDS_EVALUATE)
    if opt.evaluate_kfold is not None and opt.tile_scenes and not opt.evaluate_kfold_images:
        p.error(KFOLD_SCENES_NEED_IMAGES)
    if opt.performance is not None and (opt.evaluate is None or not opt.geocode_bboxes):
        p.error(PERFORMANCE_NEEDS_EVALUATE)
    if opt.performance is not None and opt.tile_scenes and not opt.evaluate_kfold_images:
        p.error(PERFORMANCE_SCENES_NEED_IMAGES)
    if opt.performance is not None:
        from .performance import check_options as _check_performance
        try:
            _check_performance(opt.performance_thresholds, opt.performance_eps, opt.performance_min_cages, opt.performance_rates, opt.performance_K)
        except ValueError as e:
            p.error(str(e))
    if opt.evaluate is not None:
        from .evaluate import check_kfold_options, grids_from_options
        try:
            grids_from_options(opt.evaluate_conf, opt.evaluate_eps, opt.evaluate_min_cages)
            check_kfold_options(opt.evaluate_kfold, opt.evaluate_kfold_test)
        except ValueError as e:
            p.error(str(e))
    if opt.blank_geom is not None and opt.blank_key is None:
        opt.blank_key = ""
    opt.imgsz *= 2 if len(opt.imgsz) == 1 else 1
    return opt


DEDUP_NEEDS_GEOCODE = "--dedup-years works on geocoded detections: it needs --geocode-bboxes CSV (and --save-txt --save-conf)"
DEDUP_BY_PASS = "--dedup-years keeps one year per tile and image pass: with it --facilities needs --facilities-by pass, not year"
MISSING_NEEDS_TONNAGE_DEDUP = ("--tonnage-missing adds the facilities outside a pass's imagery to the estimates of --tonnage, from the key, the outlines "
                               "and the cage_ids_min / cage_ids_max of --dedup-years: it needs both")
NEAR_SITES_NEED_TONNAGE = "--tonnage-near-sites estimates the production near the known sites with the bootstrap of --tonnage: it needs --tonnage"
KFOLD_NEEDS_EVALUATE = "--evaluate-kfold cross-validates the tuning grid of --evaluate: it needs --evaluate TRUTH_GEOJSON"
KFOLD_SCENES_NEED_IMAGES = ("--evaluate-kfold with --tile-scenes: the tiles cut from the scenes are not listed anywhere after the sweep (a tile without "
                            "a detection leaves no label file), so the image table needs --evaluate-kfold-images FILE (the tile names, one per line)")
from .land_images import NEEDS_LAND as LAND_IMAGES_NEED_LAND, SCENES_NEED_IMAGES as LAND_IMAGES_SCENES_NEED_IMAGES      # noqa: E402
from .performance import NEEDS_EVALUATE as PERFORMANCE_NEEDS_EVALUATE, SCENES_NEED_IMAGES as PERFORMANCE_SCENES_NEED_IMAGES      # noqa: E402
DEDUP_OVERLAPS_NEEDS_GEOCODE = "--dedup-overlaps needs --geocode-bboxes CSV: the download boxes whose overlaps it resolves (and --save-txt --save-conf)"
MODEL_ERRORS_NEED_GEOCODE = "--model-errors joins geocoded detections to the labels: it needs --geocode-bboxes CSV (and --save-txt --save-conf)"
MODEL_ERRORS_OR_FILE = "the model errors of --tonnage come from --model-errors or from --tonnage-errors, not from both"
FACILITY_SITES_NEED_FACILITIES = ("--facility-sites compares the facilities of --facilities with the known sites inside the download boxes: it needs "
                                  "--facilities and --geocode-bboxes CSV (and --save-txt --save-conf)")


def run_params(weights_id, conf_thres, iou_thres, max_det, imgsz, precision, save_conf, classes=None, agnostic_nms=False, augment=False,
               save_crop=False, save_img=None, blank_key=False, blank_geom=False) -> dict:
    """What the label bytes depend on (run_params.json; --resume refuses a directory written with anything else).  The optional settings are
    recorded only when set, so that the record of a run without them stays what it always was."""
    return {"weights_sha256": weights_id, "conf_thres": float(conf_thres), "iou_thres": float(iou_thres), "max_det": int(max_det),
            "imgsz": [int(v) for v in imgsz], "precision": precision, "save_conf": bool(save_conf),
            **({"classes": sorted(int(c) for c in classes)} if classes is not None else {}),
            **({"agnostic_nms": True} if agnostic_nms else {}),
            **({"augment": True} if augment else {}),
            **({"save_crop": True} if save_crop else {}),
            # annotated images are written (no --nosave): save_img = (line thickness, hide labels, hide confidences)
            **({"save_img": True, "line_thickness": int(save_img[0]), "hide_labels": bool(save_img[1]), "hide_conf": bool(save_img[2])}
               if save_img is not None else {}),
            **({"blank_key": True} if blank_key else {}),
            **({"blank_geom": True} if blank_geom else {})}


def run(weights, source, imgsz=(640, 640), conf_thres=0.25, iou_thres=0.45, max_det=1000, device="",
        save_txt=False, save_conf=False, nosave=False, classes=None, agnostic_nms=False,
        project="runs/detect", name="exp", exist_ok=False, half=False, batch_size=64, precision=None,
        workers=8, decode_threads=False, quiet=False, geocode_bboxes=None, geocode_out=None, tile_scenes=0, autotune="auto", resume=False,
        jpeg_decode="auto", augment=False, save_crop=False, line_thickness=3, hide_labels=False, hide_conf=False, blank_key=None, blank_geom=None,
        blank_geom_simplify=0.5, facilities=None, facilities_conf=0.5, facilities_eps=10.0, facilities_min_cages=5, facilities_by="year",
        land_filter=None, ocean_out=None, evaluate=None, evaluate_out=None, evaluate_conf=None, evaluate_eps=None, evaluate_min_cages=None,
        evaluate_images=None, evaluate_kfold=None, evaluate_kfold_images=None, evaluate_known_sites=None, evaluate_kfold_seed=1,
        evaluate_kfold_test=0.1, tonnage=None, tonnage_factors=None, tonnage_errors=None, tonnage_depths=None, tonnage_default_depth=4.84,
        tonnage_min_depth=1.0, tonnage_K=10000, tonnage_seed=0, tonnage_mix=0.5, bathymetry=None, bathymetry_statistic="bathy_min", dedup_years=None,
        dedup_selection="random", dedup_seed=0, model_errors=None, model_errors_conf=None, model_errors_out=None, tonnage_missing=None,
        tonnage_near_sites=None, dedup_overlaps=None, facility_sites=None, facility_sites_truth=None, facility_sites_out=None, land_images=None,
        land_images_indent=5.0, performance=None, performance_sample=None, performance_thresholds=100, performance_eps=50.0,
        performance_min_cages=5, performance_rates=None, performance_K=10000, performance_seed=0, performance_cages_per_image=5.0, log=print,
        **unsupported):
    from .engine import Engine, format_label_rows, write_label_files, jpeg_idct_rgb_checked, jpeg_slots_to_rgb, JPEG_WS_MAX, letterbox_device, letterbox_scene_tiles   # raises if the HIP library or the GPU is missing: there is no fallback

    if dedup_years is not None and not geocode_bboxes:
        raise ValueError(DEDUP_NEEDS_GEOCODE)
    if dedup_years is not None and facilities is not None and facilities_by != "pass":
        raise ValueError(DEDUP_BY_PASS)
    if dedup_years is not None and dedup_selection not in ("random", "min", "max"):
        raise ValueError(f"--dedup-selection {dedup_selection!r}: random, min or max")
    if tonnage_missing is not None and (tonnage is None or dedup_years is None):
        raise ValueError(MISSING_NEEDS_TONNAGE_DEDUP)
    if tonnage_near_sites and tonnage is None:
        raise ValueError(NEAR_SITES_NEED_TONNAGE)
    if tonnage_missing is not None:
        from .missing import parse_map
        parse_map(tonnage_missing)
    if dedup_years is not None and blank_geom is None:   # the masks of the partly blank images are their outlines
        blank_geom = ""
    if blank_geom is not None and blank_key is None:     # the outlines are made for the images the key calls partly blank
        blank_key = ""
    if facility_sites is not None and (facilities is None or not geocode_bboxes):
        raise ValueError(FACILITY_SITES_NEED_FACILITIES)
    if facilities is not None and not geocode_bboxes:
        raise ValueError("--facilities clusters geocoded detections: it needs --geocode-bboxes CSV (and --save-txt --save-conf)")
    if land_filter is not None and not geocode_bboxes:
        raise ValueError("--land-filter filters geocoded detections: it needs --geocode-bboxes CSV (and --save-txt --save-conf)")
    if land_images is not None and (land_filter is None or not geocode_bboxes):
        raise ValueError(LAND_IMAGES_NEED_LAND)
    if land_images is not None and tile_scenes and not evaluate_kfold_images:
        raise ValueError(LAND_IMAGES_SCENES_NEED_IMAGES)
    if land_images is not None:
        from .land_images import _check_indent
        _check_indent(land_images_indent)
    if dedup_overlaps is not None and not geocode_bboxes:
        raise ValueError(DEDUP_OVERLAPS_NEEDS_GEOCODE)
    if model_errors is not None and not geocode_bboxes:
        raise ValueError(MODEL_ERRORS_NEED_GEOCODE)
    if model_errors is not None and tonnage_errors:
        raise ValueError(MODEL_ERRORS_OR_FILE)
    if evaluate is not None and not geocode_bboxes:
        raise ValueError("--evaluate scores geocoded detections: it needs --geocode-bboxes CSV (and --save-txt --save-conf)")
    if evaluate_kfold is not None and evaluate is None:
        raise ValueError(KFOLD_NEEDS_EVALUATE)
    if evaluate_kfold is not None and tile_scenes and not evaluate_kfold_images:
        raise ValueError(KFOLD_SCENES_NEED_IMAGES)
    if evaluate_kfold is not None:
        from .evaluate import check_kfold_options
        check_kfold_options(evaluate_kfold, evaluate_kfold_test)
    if performance is not None and (evaluate is None or not geocode_bboxes):
        raise ValueError(PERFORMANCE_NEEDS_EVALUATE)
    if performance is not None and tile_scenes and not evaluate_kfold_images:
        raise ValueError(PERFORMANCE_SCENES_NEED_IMAGES)
    if performance is not None:
        from .performance import settings_from_options as _performance_settings
        performance_settings = _performance_settings(performance_thresholds, performance_eps, performance_min_cages, performance_rates, performance_K,
                                                     performance_seed, performance_cages_per_image)
    if tonnage is not None and not geocode_bboxes:
        raise ValueError("--tonnage estimates from geocoded detections: it needs --geocode-bboxes CSV (and --save-txt --save-conf)")
    if tonnage is not None and not tonnage_factors:
        raise ValueError("--tonnage needs --tonnage-factors FILE (pass, s_mean, s_sd, h_mean, h_sd)")
    if bathymetry and not geocode_bboxes:
        raise ValueError("--bathymetry takes the depth under geocoded facilities: it needs --geocode-bboxes CSV (and --save-txt --save-conf)")
    if bathymetry and tonnage is None and facilities is None:
        raise ValueError("--bathymetry gives the facilities of --tonnage or --facilities their depth: it needs at least one of the two")
    if bathymetry and tonnage_depths:
        raise ValueError("cage depths come from --bathymetry or from --tonnage-depths, not from both")
    for k in UNSUPPORTED:
        if unsupported.get(k):
            raise NotImplementedError(f"--{k.replace('_', '-')} is not part of the tile-sweep path (reference README.md:77)")
    save_img = not nosave                                  # [UPSTREAM detect.py] save_img = not nosave and not source.endswith('.txt')
    weights = weights[0] if isinstance(weights, (list, tuple)) else weights
    precision = precision or ("bf16" if half else "fp32")
    if augment and precision == "fp8":
        # the e4m3 activation scales are calibrated at one geometry; the augmented passes run at three (aq_engine_infer_augment refuses them)
        raise ValueError("--augment does not run with --precision fp8: its activation scales are calibrated at the tile size, and the "
                         "augmented passes run at three sizes; use --precision bf16 (or fp8w) with --augment")

    # (yolov5/detect.py has set OMP_NUM_THREADS / OPENBLAS_NUM_THREADS / MKL_NUM_THREADS to 1 before numpy and torch were loaded: the CPU
    # side of the sweep wants no thread teams; here the same for a caller that imported torch first)
    torch.set_num_threads(max(1, int(os.environ.get("AQ_CPU_THREADS", "1"))))
    rank, world, local = aqdist.init()
    multi = world > 1 or aqdist.forced()                  # the collectives run (AQ_DIST_FORCE=1: also in a world of one -- RCCL on a one-GPU box)
    dev = int(device) if str(device).strip().isdigit() else local % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(dev)

    # directories: rank 0 picks the run directory, everyone uses it
    if resume and tile_scenes:
        raise NotImplementedError("--resume works on tile directories (the manifest records tile names), not with --tile-scenes")
    if rank == 0:
        save_dir = increment_path(Path(project) / name, exist_ok=exist_ok or resume)
        (save_dir / "labels" if save_txt else save_dir).mkdir(parents=True, exist_ok=True)
        if save_crop:
            (save_dir / "crops").mkdir(exist_ok=True)
    if multi:
        box = [str(save_dir) if rank == 0 else None]
        torch.distributed.broadcast_object_list(box, src=0)
        save_dir = Path(box[0])
    labels_dir = str(save_dir / "labels")
    # done-manifest: every rank records the tiles it has finished (fsync'd per batch); --resume skips what ANY rank of the
    # interrupted run recorded (reference idiom: skip-if-exists, src/load_data/tile_tifs.py:40-41 -- which label files cannot express)
    from .manifest import DoneManifest, check_run_params, file_digest, fsync_dir, sync_filesystem_of
    durable = not tile_scenes and os.environ.get("AQ_NO_FSYNC") != "1"     # (AQ_NO_FSYNC=1: only process kills are covered, as before round 3)
    # what the label bytes depend on; --resume refuses to continue a directory written with anything else.  Collective: nobody processes
    # a tile before rank 0 has accepted the directory, and a refusal reaches every rank.
    aqdist.on_rank0(lambda: None if tile_scenes else check_run_params(
        str(save_dir), run_params(file_digest(weights) if os.path.isfile(str(weights)) else str(weights), conf_thres, iou_thres, max_det, imgsz,
                                  precision, save_conf, classes, agnostic_nms, augment, save_crop,
                                  (line_thickness, hide_labels, hide_conf) if save_img else None, blank_key is not None, blank_geom is not None),
        resume))
    done_before = DoneManifest.load(str(save_dir)) if resume else set()
    manifest = DoneManifest(str(save_dir), rank)
    if not tile_scenes:
        manifest.open()
    key_part = None
    if blank_key is not None:                              # this rank's part of the white-space key, appended batch by batch
        from . import blank as aqblank
        if not resume:                                     # (a run directory used again with --exist-ok: the earlier run's parts are not this run's)
            aqdist.on_rank0(lambda: [os.remove(str(old_)) for old_ in sorted(save_dir.glob("blank_key.rank*.csv"))] and None)
        key_part = aqblank.PartFile(str(save_dir), rank)
        key_part.open()
    geom_part = geom_bboxes = None
    if blank_geom is not None:                             # and of the partly blank images' polygons
        from . import blank_geom as aqgeom
        if not resume:
            aqdist.on_rank0(lambda: [os.remove(str(old_)) for old_ in sorted(save_dir.glob("blank_geom.rank*.jsonl"))] and None)
        if geocode_bboxes:
            from . import geocode
            geom_bboxes = geocode.load_wanted_bboxes(geocode_bboxes)
        geom_part = aqgeom.PartFile(str(save_dir), rank)
        geom_part.open()

    ck = load_checkpoint(weights)
    eng = Engine(ck, precision, dev, fp8_calibration="defer")
    if classes is not None or agnostic_nms:
        eng.set_nms_options(agnostic=agnostic_nms, classes=classes)            # [UPSTREAM non_max_suppression(pred, conf, iou, classes, agnostic_nms, max_det)]
    imgsz = check_img_size(list(imgsz), s=int(max(ck.stride)))
    try:
        # a batch some kernel cannot run is refused now, not by that kernel in the middle of the sweep; imgsz is the largest geometry the
        # letterbox produces, and every size guard grows with the tile
        eng.workspace_bytes(batch_size, *imgsz, augment=augment)
    except RuntimeError as err:
        raise SystemExit(f"--batch-size {batch_size}: {err}") from None
    if precision == "fp8":
        # e4m3 activation scales from THIS sweep's imagery and tile size (the engine's default calibrates on synthetic 640-px
        # tiles; real tiles beyond that range would saturate silently).  Rank 0 calibrates on tiles sampled across the whole file list, every
        # rank installs the same scales, and they are recorded next to run_params.json so that --resume quantises the rest of the sweep
        # exactly as the interrupted run did.
        import json
        rec = save_dir / "fp8_scales.json"

        def calibrate():
            if resume and rec.exists():
                return json.loads(rec.read_text())
            sc = eng.calibrate_fp8(_calibration_tiles(source, tile_scenes, imgsz, int(max(ck.stride)), dev))
            tmp = str(rec) + ".tmp"
            with open(tmp, "w") as f:
                json.dump(sc, f, indent=1, sort_keys=True)
                f.flush()
                os.fsync(f.fileno())
            os.replace(tmp, rec)
            return sc
        scales = aqdist.on_rank0(calibrate)
        eng.set_fp8_scales(scales)
        if rank == 0:
            log(f"fp8: {len(scales)} activation scales calibrated on this sweep's tiles (recorded in {rec}); "
                f"|t| range covered {min(scales.values()) * 448:.3g} .. {max(scales.values()) * 448:.3g}" if scales else
                "fp8: no layer of this model runs in fp8 at this geometry (bf16 throughout)")
    # decoded images go to the GPU as they are; the letterbox (resize INTER_LINEAR + pad 114) runs on the device
    if tile_scenes:
        from .scenes import SceneTiles
        dataset = SceneTiles(source, tilesize=int(tile_scenes), shard=(rank, world), workers=workers, batch_size=batch_size, pinned=True)
    else:
        dataset = LoadImages(source, img_size=imgsz, stride=int(max(ck.stride)), auto=True, shard=(rank, world), workers=workers, raw=True,
                             skip_stems=done_before)
        if resume:
            log(f"resume: {len(done_before)} tiles recorded as done in {save_dir}; rank {rank} skips {dataset.skipped} of its share")
        if save_img:                                      # cv2.imwrite picks the format by the extension; JPEG is the one written here
            other = [f for f in dataset.files if os.path.splitext(f)[1].lower() not in (".jpg", ".jpeg")]
            if other:
                raise ValueError(f"annotated images are written as JPEGs under the source's own file name: {other[0]}"
                                 f"{f' and {len(other) - 1} more' if len(other) > 1 else ''} would not be one (use --nosave)")

    # Pipeline: decode threads -> [main thread: H2D, letterbox, engine, async D2H] -> [writer thread: rescale, format, files].
    # Up to `depth` batches are in flight, each with its own workspace slot, pinned result buffers and stream.
    import queue
    import threading
    depth = max(2, int(os.environ.get("AQ_PIPELINE_DEPTH", 3)))
    streams = [torch.cuda.Stream() for _ in range(depth)]
    slot_free = [threading.Semaphore(1) for _ in range(depth)]   # a slot's pinned result buffers are reused only after its writer is done
    stats = {"seen": 0, "labels": 0, "dets": 0, "t_post": 0.0}
    gather = aqdist.DetectionGather(dev, keep=False)      # rank 0 counts what arrives; the label files are the product
    gather_lock = threading.Lock()
    flush_every = 16                                       # batches between flushes of the detection gather
    q: "queue.Queue" = queue.Queue(maxsize=depth)
    err: List[BaseException] = []

    def writer():
        try:
            if save_crop or save_img or blank_geom is not None:
                torch.cuda.set_device(dev)          # HIP's current device is per thread: the crop and image encodes and the outlines launch from here
            while True:
                item = q.get()
                if item is None:
                    return
                ev, counts_h, dets_h, paths, shapes0, hw, gidx, t_inf, slot_id, crop_src, blank_h, jflags_h = item
                item = None
                ev.synchronize()
                if jflags_h is not None and jflags_h.numpy().any():     # before anything of this batch is written or recorded
                    bad = [p for p, f in zip(paths, jflags_h.numpy().tolist()) if f]
                    raise ValueError(f"{bad[0]}: outside the acceptance rule of the GPU JPEG decode: a block's pass-1 IDCT workspace exceeds +-{JPEG_WS_MAX} "
                                     f"(dequantised coefficients no encoder produces from 8-bit pixels: a damaged quantisation table?), where libjpeg's own "
                                     f"pixels depend on its build{f'; {len(bad) - 1} more in the same batch' if len(bad) > 1 else ''}.  Use --jpeg-decode host.")
                t0 = time.perf_counter()
                nlab = ndet = 0
                released = False
                H, W = hw
                cnt = counts_h.numpy()
                det_all = dets_h.numpy()
                crops = frames = None
                key_lines = aqblank.key_rows(paths, blank_h.numpy()) if blank_h is not None else None      # (read before the slot goes back)
                geom_lines = geom_batch(paths, shapes0, gidx, blank_h.numpy(), crop_src, slot_id) if blank_geom is not None else None
                if crop_src is not None:            # before the slot goes back: its stream and arenas carry the encode
                    if save_crop:
                        crops = encode_batch_crops(det_all, cnt[:len(paths)], (H, W), shapes0, paths, crop_src, slot_id)
                    if save_img:                    # (after the crops: they are cut from the clean pixels, the drawing goes to a copy)
                        frames = encode_batch_images(det_all, cnt[:len(paths)], (H, W), shapes0, paths, crop_src, slot_id)
                    crop_src = None                 # the batch's original images may go
                written = []
                same = all(sh == shapes0[0] for sh in shapes0)       # the pinned path: one original size per batch -> one numpy pass for all tiles
                if same:
                    rows_all, offs = postprocess.batch_rows(det_all, cnt[:len(paths)], (H, W), shapes0[0])
                bulk = same and quiet and save_txt                  # a whole batch of label files in ONE C call (no interpreter lock held; round 4)
                if bulk:
                    ndet = int(offs[-1])
                    if multi and ndet:                              # the batch's rows for the detection gather, in one piece
                        cnt_b = cnt[:len(paths)].astype(np.int64)
                        keep_ = np.arange(det_all.shape[1])[None, :] < cnt_b[:, None]
                        with gather_lock:
                            gather.add(torch.from_numpy(np.repeat(np.asarray(gidx, np.int32), cnt_b)), aqdist.pack_rows(torch.from_numpy(det_all[:len(paths)][keep_].copy())))
                    # the slot's pinned result buffers have been read (batch_rows copied what it needs): hand the slot back BEFORE formatting and
                    # writing -- ~20 ms of C per batch with the synthetic checkpoint's 340 detections per tile; held across it, three slots capped the
                    # sweep at ~5.5 k tiles/s whatever the decode path (round 4)
                    slot_free[slot_id].release()
                    released = True
                    fs_fallback = durable and not can_syncfs[0]
                    nlab = write_label_files(labels_dir, [os.path.splitext(os.path.basename(p))[0] for p in paths], rows_all, offs, save_conf, fsync=fs_fallback)
                    if durable and nlab and can_syncfs[0] and not sync_filesystem_of(labels_dir):
                        can_syncfs[0] = False               # (no syncfs here: this batch's files are synced one by one now, later batches inside the C call)
                        for p in paths:
                            fp_ = os.path.join(labels_dir, os.path.splitext(os.path.basename(p))[0] + ".txt")
                            if os.path.exists(fp_):
                                fd_ = os.open(fp_, os.O_RDONLY)
                                os.fsync(fd_)
                                os.close(fd_)
                    if durable and nlab and not can_syncfs[0]:
                        fsync_dir(labels_dir)
                for b, p in enumerate(paths if not bulk else ()):
                    det = det_all[b, : cnt[b]]
                    ndet += det.shape[0]
                    rows = rows_all[offs[b]:offs[b + 1]] if same else postprocess.detections_to_rows(det, (H, W), shapes0[b])
                    if save_txt and rows.shape[0]:       # no detections => no file (the consumer relies on it)
                        f = open(os.path.join(labels_dir, os.path.splitext(os.path.basename(p))[0] + ".txt"), "wb")     # "wb": a tile processed again after a crash leaves the same bytes
                        f.write(format_label_rows(rows, save_conf))
                        f.flush()
                        written.append(f)
                        nlab += 1
                    if not quiet:
                        s = f"image {gidx[b] + 1}/{dataset.total} {p}: {H}x{W} "
                        s += postprocess.class_summary(det[:, 5], ck.names) if det.shape[0] else "(no detections), "
                        log(f"{s}{t_inf * 1e3 / len(paths):.1f}ms")
                    if multi and det.shape[0]:
                        with gather_lock:
                            gather.add(torch.full((det.shape[0],), gidx[b], dtype=torch.int32), aqdist.pack_rows(torch.from_numpy(det.copy())))
                if not released:
                    slot_free[slot_id].release()
                if crops is not None:
                    write_batch_crops(*crops)
                if frames is not None:
                    write_batch_images(*frames)
                if key_lines is not None:                   # in the part file (and on disk) before the manifest records the batch
                    key_part.append(gidx, key_lines, durable)
                if geom_lines is not None:
                    geom_part.append(*geom_lines, durable)
                # the manifest line below vouches for these bytes: on disk first (files and their directory entries), then the record -- a
                # node crash must not leave a recorded tile without its label file (it would look like "no detections" for good).
                # One syncfs per batch; per-file fsync + directory fsync where that is unavailable.
                fds = [f.fileno() for f in written]
                for f in written:
                    f.flush()
                if durable and written and not sync_filesystem_of(labels_dir):
                    for fd in fds:
                        os.fsync(fd)
                    fsync_dir(labels_dir)
                for f in written:
                    f.close()
                if not tile_scenes:
                    with manifest_lock:
                        manifest.add(Path(p).stem for p in paths)
                with lock:
                    if facilities is not None or tonnage is not None or dedup_years is not None:       # the circle areas' border test wants every image's own size
                        image_hw.update((Path(p).stem, (int(sh[0]), int(sh[1]))) for p, sh in zip(paths, shapes0))
                    stats["seen"] += len(paths)
                    stats["labels"] += nlab
                    stats["dets"] += ndet
                    stats["t_post"] += time.perf_counter() - t0
        except BaseException as e:   # surfaced by the main thread
            err.append(e)
            for sf in slot_free:     # never leave the producer blocked on a slot
                sf.release()
            while True:              # keep draining so q.put() cannot block either
                if q.get() is None:
                    return

    image_hw = {}                                          # --facilities: stem -> (h, w) of the images this rank's sweep saw
    geom_scratch = [None]                                  # one scratch for all slots (at most engine.GEOM_GROUP_SLOTS x 9 bytes), made on first use
    geom_lock = threading.Lock()

    def geom_batch(paths, shapes0, gidx, stats, src, slot_id):
        """--blank-geom (slot held): the batch's partly blank images -- known from the key's records, so a batch without one launches
        nothing -- through the component kernels on the slot's stream, in groups that bound the scratch; the winners' outer edges back in
        host memory, chained into rings.  -> (orders, part lines) of the partly blank images."""
        from .engine import blank_components, blank_geom_frame_table, blank_geom_groups, blank_ring_edges
        partly = [b for b, st in enumerate(aqblank.status(stats)) if st == aqblank.PARTLY_BLANK]
        if not partly:
            return [], []
        feats = {b: None for b in partly}                  # (no pixel below 250: "actually blank", nothing to examine)
        todo = [b for b in partly if stats[b][aqblank.FIELDS.index("nonblank_px")] > 0]
        images, bases, pitch = src
        with geom_lock, torch.cuda.stream(streams[slot_id]):
            for group in blank_geom_groups([tuple(shapes0[b]) for b in todo]):
                idx = [todo[k] for k in group]
                table = blank_geom_frame_table(np.asarray(bases, np.int64)[idx], pitch, [tuple(shapes0[b]) for b in idx])
                rec_dev, geom_scratch[0], table_dev = blank_components(images, table, scratch=geom_scratch[0])
                rec = rec_dev.cpu().numpy()
                edges = blank_ring_edges(table, rec, rec_dev, geom_scratch[0], table_dev)     # (waits for the stream: the scratch is free again)
                for b, r, e in zip(idx, rec, edges):
                    if r[1] > 0:
                        feats[b] = aqgeom.feature(paths[b], r, aqgeom.ring_from_edges(e, int(shapes0[b][1])), geom_bboxes, blank_geom_simplify)
        return [gidx[b] for b in partly], aqgeom.part_rows([paths[b] for b in partly], [feats[b] for b in partly])

    crops_dir = str(save_dir / "crops")
    crop_arena = [None] * depth                            # per slot: (device int16, pinned int16) coefficient arenas, made on first use

    def encode_batch_crops(det_all, cnt, hw, shapes0, paths, crop_src, slot_id):
        """--save-crop, first half (slot held): upstream's crop rectangles and names for the batch, the encode kernel on the slot's stream,
        the used part of the arena back in host memory.  -> (coefficients, crop table, paths relative to save_dir) or None."""
        from .engine import CROP_ARENA_BLOCKS, crop_blocks, crop_table, encode_crops
        images, bases, pitch = crop_src
        groups = {}
        for b, sh in enumerate(shapes0):                  # (one original size per batch in practice; tiles of another size in turn)
            groups.setdefault(tuple(sh), []).append(b)
        tiles_, rects_, rel = [], [], []
        for sh, idx in groups.items():
            idx = np.asarray(idx)
            tile, cls, rects, ordinal = postprocess.batch_crops(det_all[idx], cnt[idx], hw, sh)
            tiles_.append(idx[tile])
            rects_.append(rects)
            for t_, c_, k_ in zip(idx[tile].tolist(), cls.tolist(), ordinal.tolist()):
                rel.append(f"crops/{ck.names[c_]}/{postprocess.crop_file_name(Path(paths[t_]).stem, k_)}")
        if not rel:
            return None
        table = crop_table(np.asarray(bases, np.int64)[np.concatenate(tiles_)], pitch, np.concatenate(rects_))
        need = max(CROP_ARENA_BLOCKS, int(crop_blocks(table).max()))
        with torch.cuda.stream(streams[slot_id]):
            if crop_arena[slot_id] is None or crop_arena[slot_id][0].numel() < need * 192:
                crop_arena[slot_id] = (torch.empty(need * 192, dtype=torch.int16, device=dev), torch.empty(need * 192, dtype=torch.int16, pin_memory=True))
            coef, table = encode_crops(images, table, arena_blocks=crop_arena[slot_id][0].numel() // 192, arena=crop_arena[slot_id][0],
                                       arena_host=crop_arena[slot_id][1])
        return coef, table, rel

    def write_batch_crops(coef, table, rel):
        """--save-crop, second half (slot free): Huffman coding and files in one C call on four threads, then on disk before the manifest
        records the batch (syncfs; per-file fsync and directory fsyncs where that is unavailable)."""
        from .engine import write_crop_files
        write_crop_files(str(save_dir), rel, coef, table, threads=4, fsync=durable and not can_syncfs[0])
        if durable and not (can_syncfs[0] and sync_filesystem_of(crops_dir)):
            if can_syncfs[0]:
                can_syncfs[0] = False
                for r_ in rel:
                    fd_ = os.open(os.path.join(str(save_dir), r_), os.O_RDONLY)
                    os.fsync(fd_)
                    os.close(fd_)
            for d_ in sorted({os.path.dirname(r_) for r_ in rel}):
                fsync_dir(os.path.join(str(save_dir), d_))
            fsync_dir(crops_dir)

    img_scratch = [None] * depth                           # per slot: the batch's annotated copies (uint8 CUDA)
    frame_arena = [None] * depth                           # per slot: (device int16, pinned int16) coefficient arenas of the frame encoder
    label_atlas = [None]
    checked_sizes = set()

    def encode_batch_images(det_all, cnt, hw, shapes0, paths, img_src, slot_id):
        """Annotated images, first half (slot held): upstream's boxes and labels for the batch as primitives binned per cell, the draw kernel
        (source -> annotated copies in the slot's scratch), the 4:2:0 encode kernel on the copies, the coefficients back in host memory.
        -> (coefficients, frame table, file names relative to save_dir)."""
        from . import annotate
        from .engine import (FRAME_ARENA_MCUS, PRIM_DTYPE, annotate_images, canvas_table, encode_frames, frame_mcus, frame_table,
                             image_save_bytes)
        images, bases, pitch = img_src
        if label_atlas[0] is None:
            label_atlas[0] = annotate.LabelAtlas(dev)
        sizes = np.asarray([tuple(sh) for sh in shapes0], np.int64)
        for sh in {tuple(sh) for sh in shapes0} - checked_sizes:      # a batch whose copies cannot be held is refused by name, once per size
            checked_sizes.add(sh)
            need, free = image_save_bytes(batch_size, *sh), torch.cuda.mem_get_info(dev)[0]
            if img_scratch[slot_id] is None and need > free:
                raise SystemExit(f"--batch-size {batch_size}: writing annotated {sh[1]}x{sh[0]} images takes {need >> 20} MiB per pipeline slot, "
                                 f"{free >> 20} MiB are free (use a smaller batch or --nosave)")
        groups = {}
        for b, sh in enumerate(shapes0):                  # (one original size per batch in practice; tiles of another size in turn)
            groups.setdefault(tuple(sh), []).append(b)
        parts = []
        for sh, idx in groups.items():
            idx = np.asarray(idx)
            tile, cls, conf, xyxy = postprocess.batch_boxes(det_all[idx], cnt[idx], hw, sh)
            labels = None
            if not hide_labels:
                labels = label_atlas[0].lookup(postprocess.label_strings(ck.names, cls, conf, hide_conf), annotate.font_size(*sh))
            parts.append(postprocess.annotation_prims(idx[tile], cls, xyxy, sizes, annotate.line_width(*sh, line_thickness), labels))
        P = {f: np.concatenate([p_[0][f] for p_ in parts]) for f in postprocess.PRIM_FIELDS}
        owner = np.concatenate([p_[1] for p_ in parts])
        order = np.argsort(owner, kind="stable")          # (groups of sizes interleave in the batch; inside an image the order stays upstream's)
        P, owner = {f: v[order] for f, v in P.items()}, owner[order]
        cell_start, cell_prims = postprocess.bin_prims(P, owner, sizes)
        canvases, nbytes = canvas_table(np.asarray(bases, np.int64), pitch, sizes)
        table = frame_table(canvases["dst"], canvases["dst_pitch"], sizes)
        need = max(FRAME_ARENA_MCUS, int(frame_mcus(table).max()))
        with torch.cuda.stream(streams[slot_id]):
            if img_scratch[slot_id] is None or img_scratch[slot_id].numel() < nbytes:
                img_scratch[slot_id] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            if frame_arena[slot_id] is None or frame_arena[slot_id][0].numel() < need * 384:
                frame_arena[slot_id] = (torch.empty(need * 384, dtype=torch.int16, device=dev), torch.empty(need * 384, dtype=torch.int16, pin_memory=True))
            atlas = label_atlas[0].device_atlas()
            annotate_images(images, canvases, postprocess.prims_array(P, PRIM_DTYPE), cell_start, cell_prims, atlas, nbytes, out=img_scratch[slot_id])
            coef, table = encode_frames(img_scratch[slot_id], table, arena_mcus=frame_arena[slot_id][0].numel() // 384, arena=frame_arena[slot_id][0],
                                        arena_host=frame_arena[slot_id][1])
        return coef, table, [image_file_name(p_) for p_ in paths]

    def image_file_name(path):
        """[UPSTREAM detect.py] save_path = save_dir / p.name; a scene's tiles: the label file's stem + the extension of the reference's tile jpegs
        (reference src/load_data/tile_tifs.py: tif_name.replace('.tif', '.jpeg'))."""
        return os.path.splitext(os.path.basename(path))[0] + ".jpeg" if tile_scenes else os.path.basename(path)

    def write_batch_images(coef, table, rel):
        """Annotated images, second half (slot free): Huffman coding and files in one C call on four threads, then on disk before the manifest
        records the batch, as the crops are."""
        from .engine import write_image_files
        write_image_files(str(save_dir), rel, coef, table, threads=4, fsync=durable and not can_syncfs[0])
        if durable and not (can_syncfs[0] and sync_filesystem_of(str(save_dir))):
            if can_syncfs[0]:
                can_syncfs[0] = False
                for r_ in rel:
                    fd_ = os.open(os.path.join(str(save_dir), r_), os.O_RDONLY)
                    os.fsync(fd_)
                    os.close(fd_)
            fsync_dir(str(save_dir))

    lock = threading.Lock()
    manifest_lock = threading.Lock()
    can_syncfs = [True]
    n_writers = max(4, min(8, workers // 2)) if quiet else 1          # (per-image log lines stay in order with a single writer; the quiet path's work is C without the interpreter lock)
    depth_q = depth
    wts = [threading.Thread(target=writer, daemon=True) for _ in range(n_writers)]
    for w_ in wts:
        w_.start()
    t_pre = t_inf = 0.0
    t_start = time.perf_counter()
    shape_str = ""
    pinned = [None] * depth
    k = 0
    def scene_source():
        """Scene mode: (tile names, ("scene", path, raster, origins, (h, w)), shapes, None, global tile indices) per batch."""
        for path, arr, stems, origins, hw, gids in dataset.batches():
            names = [os.path.join(os.path.dirname(path), st_ + ".tif") for st_ in stems]     # label file = <tile stem>.txt
            yield names, ("scene", path, arr, origins, hw), [hw] * len(stems), None, gids

    gpu_superbatch = max(batch_size, int(os.environ.get("AQ_JPEG_GPU_SUPERBATCH", 2048)) // batch_size * batch_size)

    def gpu_jpeg_source(sub):
        """--jpeg-decode gpu: (paths, ("gpu_coef", coef int16 CUDA [b * nco], qt int16 CUDA [b, 192], decode-done event, done-hook, ...), shapes,
        None) per batch.  D + 2 super-batch buffers rotate: while the engine consumes the batches of super-batch k, the Huffman kernels of
        k + 1 .. k + D run (one launch each: a launch takes as long as its slowest image's serial decode, 50-200 ms for 1024-px tiles,
        whatever the number of tiles in it) and C threads read and prepare the files of k + 3 (aq_jpeg_prepare_files)."""
        from concurrent.futures import ThreadPoolExecutor
        from . import jpeg as aqjpeg
        from .engine import jpeg_huffman_decode
        W0, H0 = aqjpeg.scan_file(sub.files[0])
        nco = aqjpeg.coef_count(H0, W0)
        D = max(1, int(os.environ.get("AQ_JPEG_GPU_INFLIGHT", 3)))     # decode launches in flight ahead of the one being consumed
        NB = D + 2
        SB = min(gpu_superbatch, (len(sub.files) + batch_size - 1) // batch_size * batch_size)
        per = aqjpeg.stream_capacity(H0, W0)
        if SB * per + 256 >= 1 << 32:
            raise ValueError("--jpeg-decode gpu: AQ_JPEG_GPU_SUPERBATCH x bytes per image exceeds 4 GiB; lower it")
        # super-batches ramp up (4 x batch, 8 x batch, ... SB): the first tiles reach the engine after one small decode launch instead of a
        # full one -- a launch takes as long as its slowest image whatever its size, so small launches only cost throughput at the start
        chunks, s_, size = [], 0, min(SB, 4 * batch_size)
        while s_ < len(sub.files):
            chunks.append(sub.files[s_:s_ + size])
            s_ += size
            size = min(SB, size * 2)
        NB = min(NB, len(chunks))
        # Buffer set i is created when super-batch i is first prepared -- the pool thread is already reading files into set 0 while the main
        # thread allocates set 1 -- and sized for the largest super-batch it will ever hold (i, i + NB, ...: the ramp's small ones stay small
        # in a short sweep).  Pinned memory is allocated as such (torch.empty(pin_memory=True)): `zeros().pin_memory()` touched and copied
        # 2.7 GB at start-up, 1.4 of the 2.0 s the mode lost to the split path before its first batch (65 k-image sweep, round 4).
        host, batches_h, dev_streams, dev_coef, status_h = [None] * NB, [None] * NB, [None] * NB, [None] * NB, [None] * NB

        def make_set(i):
            cap = max(len(chunks[k_]) for k_ in range(i, len(chunks), NB))
            cap = (cap + batch_size - 1) // batch_size * batch_size
            host[i] = torch.empty(cap * per + 256, dtype=torch.uint8, pin_memory=True)
            host[i][-256:].zero_()
            batches_h[i] = aqjpeg.GpuDecodeBatch(cap, H0, W0, stream_buf=host[i].numpy(), bytes_per_image=per)
            dev_streams[i] = torch.empty(cap * per + 256, dtype=torch.uint8, device=dev)
            dev_coef[i] = torch.empty(cap * nco, dtype=torch.int16, device=dev)
            status_h[i] = torch.zeros(cap * aqjpeg.GpuDecodeBatch.SEG_CAP, dtype=torch.int32, pin_memory=True)
        dstreams = [torch.cuda.Stream() for _ in range(NB)]
        consumed = [[] for _ in range(NB)]                 # events of the batches that read buffer i: its next decode waits for them
        nthreads = max(2, min(sub.workers, 16))
        pool = ThreadPoolExecutor(1)                       # one orchestrating thread; the parallelism is inside the C call

        def launch(k, prepared):
            i = k % NB
            segs, sets, first = prepared
            n = len(chunks[k])
            ds = dstreams[i]
            for ev_ in consumed[i]:
                ds.wait_event(ev_)
            consumed[i] = []
            with torch.cuda.stream(ds):
                used = (int(segs["stream_off"][-1]) + int(segs["stream_len"][-1]) + 256 + 127) // 128 * 128
                dev_streams[i][:used].copy_(host[i][:used], non_blocking=True)
                segs_d = torch.from_numpy(segs.view(np.uint8).reshape(-1, 32)).pin_memory().to(dev, non_blocking=True)
                sets_d = torch.from_numpy(np.ascontiguousarray(sets)).pin_memory().to(dev, non_blocking=True)
                qt_d = torch.from_numpy(batches_h[i].qt[:n].view(np.int16).reshape(n, 192).copy()).pin_memory().to(dev, non_blocking=True)
                dev_coef[i][:n * nco].zero_()
                st_d = torch.empty(segs.shape[0], dtype=torch.int32, device=dev)
                jpeg_huffman_decode(dev_streams[i], segs_d, sets_d, dev_coef[i], st_d)
                status_h[i][:segs.shape[0]].copy_(st_d, non_blocking=True)
                ev_ = torch.cuda.Event()
                ev_.record(ds)
            return ev_, qt_d, first, segs.shape[0], (segs_d, sets_d, st_d)

        try:
            futures, launched = {}, {}
            next_prep = next_launch = 0
            for k in range(len(chunks)):
                while next_prep < len(chunks) and next_prep < k + NB:          # (buffer next_prep % NB was last used by super-batch next_prep - NB < k)
                    if host[next_prep % NB] is None:
                        make_set(next_prep % NB)
                    futures[next_prep] = pool.submit(batches_h[next_prep % NB].prepare_files, chunks[next_prep], nthreads)
                    next_prep += 1
                while next_launch < len(chunks) and next_launch <= k + D:
                    launched[next_launch] = launch(next_launch, futures.pop(next_launch).result())
                    next_launch += 1
                ev_, qt_d, first, nseg, keep = launched.pop(k)
                ev_.synchronize()                                              # this super-batch's coefficients are in HBM; its statuses on the host
                st = status_h[k % NB][:nseg].numpy()
                if st.any():
                    bad_seg = int(np.nonzero(st)[0][0])
                    bad_img = int(np.searchsorted(first, bad_seg, side="right") - 1)
                    raise ValueError(f"{chunks[k][bad_img]}: corrupt JPEG scan (GPU entropy decode status {int(st[bad_seg])}; libjpeg / Pillow refuse "
                                     "the file as truncated)")
                i = k % NB
                paths_k = chunks[k]
                for s_ in range(0, len(paths_k), batch_size):
                    b_ = min(batch_size, len(paths_k) - s_)
                    hook = (lambda e, i=i: consumed[i].append(e))
                    yield (paths_k[s_:s_ + b_], ("gpu_coef", dev_coef[i][s_ * nco:(s_ + b_) * nco], qt_d[s_:s_ + b_], ev_, hook, (H0, W0), nco),
                           [(H0, W0)] * b_, None)
        finally:
            pool.shutdown(wait=False)

    def image_source():
        """Every header is read once (no decode): the images of the most common size take the zero-copy pinned path, any others
        (the reference's tiler cuts smaller edge tiles for scenes that are not a multiple of 1024, src/load_data/tile_tifs.py:35-36)
        follow through the generic path, grouped by size -- a stray size can no longer end the sweep half way."""
        parts = []
        if len(dataset):
            try:
                sizes = None
                if jpeg_decode != "host" and not decode_threads:       # one header pass serves both questions when every file qualifies
                    split_sizes = dataset.scan_split_decodable()
                    if all(r is not None for r in split_sizes):
                        sizes, all_split[0] = split_sizes, True
                if sizes is None:
                    sizes = dataset.scan_sizes()
                main, odd = size_parts(sizes)
            except Exception as e:                       # unreadable header: let the generic path report the file
                log(f"note: header scan failed ({e}); using the generic loader")
                main, odd = [], list(range(len(dataset)))
            if main:
                parts.append((dataset.subset(main), True))
            if odd:
                log(f"note: {len(odd)} of {len(dataset)} images differ in size from the rest; they take the generic loader")
                parts.append((dataset.subset(odd), False))
        for sub, fast in parts:
            if fast:
                # split JPEG decode (Huffman on the host, the rest on the GPU) when every file of this part is a baseline 4:2:0 JPEG
                split = False
                if jpeg_decode != "host" and not decode_threads:
                    split = all_split[0] or split_decodable(sub, jpeg_decode)
                if jpeg_decode == "gpu" and not split:
                    raise ValueError("--jpeg-decode gpu needs baseline 4:2:0 JPEGs throughout (use auto or host)")
                use_gpu = jpeg_decode == "gpu" or (jpeg_decode == "auto" and split and len(sub) >= int(os.environ.get("AQ_JPEG_GPU_AUTO_MIN", 32768)))
                if split and not split_note[0]:
                    split_note[0] = True
                    log(f"jpeg decode: split (entropy decoding in {sub.workers} worker processes, IDCT / upsampling / colour conversion on the GPU)"
                        if not use_gpu else
                        f"jpeg decode: gpu (entropy decoding on the GPU, one lane per image, super-batches of {gpu_superbatch} tiles; "
                        f"{sub.workers} reader threads strip byte stuffing; IDCT / upsampling / colour conversion on the GPU)")
                if use_gpu:
                    it = gpu_jpeg_source(sub)
                else:
                    gen = sub.pinned_batches(batch_size, depth + 2, processes=0 if decode_threads else None, coef=split)     # one buffer more than the batches in flight: the workers decode one batch ahead
                    release_of[0] = lambda i, sub=sub: sub.release(i)
                    it = gen
            else:
                it = ((p_, torch.from_numpy(b_).pin_memory(), s_, None) for p_, b_, s_ in sub.batches(batch_size))
            n_ = 0
            for p_, h_, s_, bi_ in it:
                yield p_, h_, s_, bi_, sub.indices[n_: n_ + len(p_)]
                n_ += len(p_)

    def original_images(tiles0):
        """--save-crop, the annotated images and --blank-key: the batch's decoded tiles (uint8 CUDA [B, H0, W0, 3]) as the crop and frame
        encoders and the statistics kernel address them; None when none of them is asked for."""
        if not (save_crop or save_img or blank_key is not None):
            return None
        B_, H0_, W0_, _ = tiles0.shape
        return tiles0.view(-1), [b_ * H0_ * W0_ * 3 for b_ in range(B_)], W0_ * 3

    blank_slot = [None] * depth                            # per slot: scratch, records, pinned records, frame table on the device and its bytes

    def blank_batch(src, shapes0, slot):
        """--blank-key: the statistics kernel over the batch's source images on the slot's stream, the records (36 bytes per image) on their
        way to the slot's pinned buffer.  -> int32 pinned [B, 9], valid once the batch's event has passed."""
        from .engine import BLANK_FIELDS, blank_frame_table, blank_stats
        images, bases, pitch = src
        table = blank_frame_table(np.asarray(bases, np.int64), pitch, np.asarray([tuple(sh) for sh in shapes0], np.int64))
        n = table.shape[0]
        need = int(eng.lib.aq_blank_stats_scratch_bytes(table.ctypes.data, n))
        bs = blank_slot[slot]
        if bs is None or bs["scratch"].numel() < need or bs["out"].shape[0] < n:
            bs = blank_slot[slot] = {"scratch": torch.empty(max(need, 4), dtype=torch.uint8, device=dev),
                                     "out": torch.empty((max(n, batch_size), len(BLANK_FIELDS)), dtype=torch.int32, device=dev),
                                     "host": torch.empty((max(n, batch_size), len(BLANK_FIELDS)), dtype=torch.int32).pin_memory(),
                                     "table": None, "table_bytes": None}
        if bs["table_bytes"] != table.tobytes():           # (batch after batch of one tile size: the table is uploaded once per slot)
            bs["table"], bs["table_bytes"] = torch.from_numpy(table.view(np.uint8).copy()).to(dev), table.tobytes()
        out = blank_stats(images, table, scratch=bs["scratch"], out=bs["out"], frames_dev=bs["table"])
        bs["host"][:n].copy_(out, non_blocking=True)
        return bs["host"][:n]

    release_of = [None]
    split_note = [False]
    t_steady, n_steady, n_fed = [None], [0], [0]
    all_split = [False]
    jpeg_scratch = [None] * depth
    jpeg_flags = [None] * depth                            # per slot: the pixel half's acceptance flags, on the device and pinned

    def jpeg_flag_slot(slot):
        if jpeg_flags[slot] is None:
            jpeg_flags[slot] = (torch.empty(batch_size, dtype=torch.int32, device=dev), torch.empty(batch_size, dtype=torch.int32).pin_memory())
        return jpeg_flags[slot]
    source_iter = scene_source() if tile_scenes else image_source()
    scene_dev, scene_path, scene_ev = None, None, None
    # Autotune on the first full batch (rank 0 times, every rank installs the same table: identical kernels on all GPUs of a run).
    per_rank = dataset.total // max(world, 1)
    tune = autotune == "on" or (autotune == "auto" and per_rank >= 8 * batch_size)
    if tune and world > 1 and ((dataset.n_scenes_total if tile_scenes else dataset.total) < world or resume):
        tune = False                                   # some rank may have no batch to meet the broadcast with
    tune_cache = os.environ.get("AQ_TUNE_CACHE") or os.path.join(os.path.expanduser("~"), ".cache", "aquaculture_amd", "tune.json")
    copy_done = []
    diag = {"source": 0.0, "slot_wait": 0.0, "put": 0.0, "writer_busy": 0.0} if os.environ.get("AQ_E2E_DIAG") == "1" else None
    t_src = time.perf_counter()
    try:
        for paths, host, shapes0, buf_i, gidx in source_iter:
            if err:
                break
            t0 = time.perf_counter()
            if diag is not None:
                diag["source"] += t0 - t_src
            slot = k % depth
            slot_free[slot].acquire()
            if diag is not None:
                diag["slot_wait"] += time.perf_counter() - t0
            st = streams[slot]
            crop_src = jflags = jflags_h = None
            with torch.cuda.stream(st):
                if isinstance(host, tuple) and host[0] == "scene":      # scene mode: one upload per scene, tiles cut by the letterbox kernel
                    _, spath, sarr, origins, thw = host
                    if spath != scene_path:                # page-locked source: async copy, its buffer goes back once the copy is done
                        scene_dev, scene_path = torch.from_numpy(sarr).to(dev, non_blocking=True), spath
                        scene_ev = torch.cuda.Event()
                        scene_ev.record(st)
                        dataset.uploaded(dataset.slot_of[spath], scene_ev)
                    else:
                        st.wait_event(scene_ev)            # another stream uploaded this scene
                    scene_dev.record_stream(st)
                    if save_crop or save_img or blank_key is not None:     # the crops are cut from the raster: tile b's pixel (x, y) at its origin + (x, y)
                        row_b = int(scene_dev.shape[1]) * 3
                        crop_src = (scene_dev.view(-1), [y0 * row_b + x0 * 3 for x0, y0 in origins], row_b)
                    tiles = letterbox_scene_tiles(scene_dev, origins, thw, tuple(imgsz), int(max(ck.stride)), True)
                elif isinstance(host, tuple) and host[0] == "gpu_coef":   # --jpeg-decode gpu: the coefficient blocks are in HBM already
                    _, coef_v, qt_v, dec_ev, hook, (h0_, w0_), nco_ = host
                    st.wait_event(dec_ev)
                    if jpeg_scratch[slot] is None:
                        jpeg_scratch[slot] = torch.empty(eng.lib.aq_jpeg_scratch_bytes(batch_size, h0_, w0_), dtype=torch.uint8, device=dev)
                    off_ = torch.arange(qt_v.shape[0], dtype=torch.int64, device=dev) * nco_
                    tiles, jflags = jpeg_idct_rgb_checked(coef_v, off_, qt_v, h0_, w0_, scratch=jpeg_scratch[slot], flags=jpeg_flag_slot(slot)[0])
                    used_ev = torch.cuda.Event()
                    used_ev.record(st)
                    hook(used_ev)                          # the super-batch's buffer is free for its next decode once this batch has read it
                    crop_src = original_images(tiles)
                    tiles = letterbox_device(tiles, tuple(imgsz), int(max(ck.stride)), True)
                else:
                    tiles = host.to(dev, non_blocking=True)
                    if buf_i is not None:                  # hand the pinned buffer back once its H2D copy has completed
                        h2d = torch.cuda.Event()
                        h2d.record(st)
                        copy_done.append((h2d, buf_i))
                    if tiles.dim() == 2:                   # coefficient blocks from the split JPEG decode: the pixel half runs here
                        h0_, w0_ = shapes0[0]
                        if jpeg_scratch[slot] is None:
                            jpeg_scratch[slot] = torch.empty(eng.lib.aq_jpeg_scratch_bytes(batch_size, h0_, w0_), dtype=torch.uint8, device=tiles.device)
                        tiles, jflags = jpeg_slots_to_rgb(tiles, h0_, w0_, scratch=jpeg_scratch[slot], flags=jpeg_flag_slot(slot)[0])
                    crop_src = original_images(tiles)
                    tiles = letterbox_device(tiles, tuple(imgsz), int(max(ck.stride)), True)
                blank_h = blank_batch(crop_src, shapes0, slot) if blank_key is not None else None
                if not (save_crop or save_img or blank_geom is not None):
                    crop_src = None                        # (only the statistics read the source: the writer gets the records, not the pixels)
                if tune:                                   # once, before the pipeline fills
                    tune = False
                    geom = [int(tiles.shape[0]), int(tiles.shape[1]), int(tiles.shape[2])]
                    t_tune = time.perf_counter()
                    # (--augment: the tables of the three passes' geometries, [((B, Hp, Wp), cfgs)]; the plain table last, as get_conv_config reports it)
                    box = [geom, (eng.autotune(tiles, cache=tune_cache, augment=True) if augment else eng.autotune(tiles, cache=tune_cache))
                           if rank == 0 else None]
                    if multi:
                        torch.distributed.broadcast_object_list(box, src=0)
                        if rank != 0 and box[0] == geom:
                            for g_, cfgs_ in (box[1] if augment else [(geom, box[1])])[::-1]:
                                eng.set_tuned_table(*g_, cfgs_)
                    if rank == 0:
                        n_tuned = sum(1 for c in (box[1][0][1] if augment else box[1]) if c >= 0)
                        log(f"autotuned {n_tuned} conv layers for batch {geom[0]} x {geom[1]}x{geom[2]}"
                            f"{' and the augmented passes ' + ', '.join(f'{g_[1]}x{g_[2]}' for g_, _ in box[1][1:]) if augment else ''} in "
                            f"{time.perf_counter() - t_tune:.1f}s (table: {tune_cache})")
                t1 = time.perf_counter()
                dets, counts = eng.infer(tiles, conf_thres, iou_thres, max_det, slot=slot, augment=augment)
                B = tiles.shape[0]
                if pinned[slot] is None or pinned[slot][0].shape[0] < B:
                    pinned[slot] = (torch.empty((max(B, batch_size),), dtype=torch.int32).pin_memory(),
                                    torch.empty((max(B, batch_size), max_det, 6), dtype=torch.float32).pin_memory())
                counts_h, dets_h = pinned[slot][0][:B], pinned[slot][1][:B]
                counts_h.copy_(counts, non_blocking=True)
                dets_h.copy_(dets, non_blocking=True)
                if jflags is not None:                     # the acceptance flags of the JPEG pixel half travel with the results the writer waits for
                    jflags_h = jpeg_flag_slot(slot)[1][:B]
                    jflags_h.copy_(jflags, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(st)
            H, W = int(tiles.shape[1]), int(tiles.shape[2])
            shape_str = f"(1, 3, {H}, {W})"
            t2 = time.perf_counter()
            q.put((ev, counts_h, dets_h, paths, shapes0, (H, W), list(gidx), t2 - t1, slot, crop_src, blank_h, jflags_h))
            crop_src = None
            if diag is not None:
                diag["put"] += time.perf_counter() - t2
            n_fed[0] += len(paths)
            while copy_done and (copy_done[0][0].query() or len(copy_done) > depth):
                ev_, bi_ = copy_done.pop(0)
                ev_.synchronize()
                (release_of[0] or dataset.release)(bi_)
            t_pre += t1 - t0
            t_inf += t2 - t1
            k += 1
            if k == 2:                                     # steady state: from the hand-over of the second batch (header scan, worker start-up,
                t_steady[0], n_steady[0] = time.perf_counter(), sum(1 for _ in gidx)        # autotune and the pipeline fill are behind us)
            if multi and k % flush_every == 0:         # bounded gather: rows leave the host lists every few batches (collective)
                with gather_lock:
                    gather.flush(more=True, failed=bool(err))
            t_src = time.perf_counter()
    except BaseException as e:   # anything the main loop raises (engine, autotune, a decode error, another rank's RankFailed) ends the sweep
        err.append(e)            # HERE, but only after the writers are joined and the other ranks have been told (the collective tail below)
    for _ in wts:
        q.put(None)
    for w_ in wts:
        w_.join()
    if key_part is not None:
        # every row of this rank is in its part file now; rank 0 merges all parts of the directory after the counters' all-reduce below, which
        # no rank passes before every rank has come this far (a resumed run finds the interrupted run's parts too)
        key_part.close()
    if geom_part is not None:
        geom_part.close()
    if multi:                                          # collective tail; a failed rank takes the others down with it at once
        try:
            with gather_lock:
                gather.finish(failed=bool(err))
        except aqdist.RankFailed:
            if not err:                                # another rank failed: that IS this rank's error
                raise
    if err:                                            # this rank's own error, with its traceback (not the RankFailed its flag just raised here too)
        raise err[0]
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t_start
    seen, n_labels, n_dets, t_post = stats["seen"], stats["labels"], stats["dets"], stats["t_post"]

    if multi:       # the one collective of the path (detection gather over RCCL/xGMI) has run in bounded pieces; now the counters
        seen_all, labels_all, dets_all, elapsed = aqdist.reduce_counters(seen, n_labels, n_dets, elapsed, dev)
        assert rank != 0 or gather.total == dets_all, "gathered detection rows do not add up"
    else:
        seen_all, labels_all, dets_all = seen, n_labels, n_dets
    if rank == 0:
        per = lambda t: t * 1e3 / max(seen, 1)
        log(f"Speed: {per(t_pre):.1f}ms pre-process, {per(t_inf):.1f}ms inference, {per(t_post):.1f}ms NMS-out/post-process "
            f"per image at shape {shape_str} (host time per stage; stages overlap)")
        log(f"{seen_all} images, {dets_all} detections, {seen_all / max(elapsed, 1e-9):.1f} images/s on {world} GPU(s) [{precision}]")
        if diag is not None:
            log(f"diag (main thread, seconds of {elapsed:.2f}): waiting for the source {diag['source']:.2f}, for a free slot {diag['slot_wait']:.2f}, "
                f"in q.put {diag['put']:.2f}, pre {t_pre:.2f}, enqueue {t_inf:.2f}; writers' post time summed over threads {t_post:.2f}")
        if t_steady[0] is not None and seen > 4 * batch_size:
            # this rank's rate once the sweep is under way (everything up to the second batch -- header scan, decode worker start-up,
            # tile-configuration timing, pipeline fill -- excluded): what a long sweep converges to
            t_end = t_start + (time.perf_counter() - t_start if world > 1 else elapsed)
            log(f"steady state: {(seen - 2 * batch_size) / max(t_end - t_steady[0], 1e-9):.1f} images/s on this GPU after the first two batches")
        if save_txt or save_img:                           # [UPSTREAM detect.py] the closing line names the run directory
            log(f"Results saved to {save_dir}" + (f"\n{labels_all} labels saved to {save_dir / 'labels'}" if save_txt else ""))
        if blank_key is not None:
            key_out = blank_key or str(save_dir / aqblank.KEY_FILE)
            listing = None
            if not tile_scenes:
                from .dataloader import list_images
                listing = list_images(source)
            n_key = aqblank.merge_parts(str(save_dir), key_out, listing)
            log(f"blank key: {n_key[aqblank.BLANK]} blank, {n_key[aqblank.PARTLY_BLANK]} partly blank, {n_key[aqblank.COMPLETE]} complete "
                f"images in {key_out}")
        if blank_geom is not None:
            geom_out = blank_geom or str(save_dir / aqgeom.GEOM_FILE)
            n_geom = aqgeom.merge_parts(str(save_dir), geom_out, listing, crs="urn:ogc:def:crs:EPSG::3857" if geom_bboxes is not None else None)
            log(f"blank geom: {n_geom['features']} polygons of partly blank images in {geom_out}; {len(n_geom['actually_blank'])} actually blank"
                + (": " + " ".join(n_geom["actually_blank"]) if n_geom["actually_blank"] else ""))
        if geocode_bboxes:
            # the consumer's next step (reference src/process_yolo/geocode_results.py:106-197) on the label files just written
            if not save_txt or not save_conf:
                raise ValueError("--geocode-bboxes reads the label files: it needs --save-txt --save-conf")
            from . import geocode
            t_g = time.perf_counter()
            out = geocode_out or str(save_dir / "detections.geojson")
            table = geocode.geocode_label_dir(labels_dir, geocode_bboxes, out)
            log(f"{table['image'].shape[0]} detections geocoded to {out} in {time.perf_counter() - t_g:.2f}s")
            ocean = None
            unique = None                                  # --dedup-overlaps' survivors alone: what --performance's first curve sees
            if dedup_overlaps is not None:
                # the reference's next statement (geocode_results.py:256-262): every cage once where the download boxes overlap.  The
                # survivors are the one keep mask of every later step; detections.geojson stays as it is
                from . import overlaps as aqover
                t_o = time.perf_counter()
                ov_out = dedup_overlaps or str(save_dir)
                ov = aqover.dedup_from_table(table, geocode_bboxes, ov_out)
                ocean = unique = ov["keep"]
                log(f"dedup overlaps: {aqover.describe(ov['summary'])} in {ov_out} in {time.perf_counter() - t_o:.2f}s")
            if land_filter is not None:
                # the step between them (reference geocode_results.py:200-218, :267-271): detections.geojson stays as it is
                from . import land as aqland
                t_l = time.perf_counter()
                segs = aqland.load_land_geojson(land_filter)
                at_sea = aqland.ocean_rows(table, segs)
                ocean = at_sea if ocean is None else ocean & at_sea       # with --dedup-overlaps: both unique and at sea
                ocean_path = ocean_out or str(save_dir / "ocean_detections.geojson")
                n_ocean = aqland.write_ocean_geojson(ocean_path, table["stems"], table, ocean)
                log(f"{n_ocean} of {ocean.shape[0]} detections at sea ({segs.shape[0]} land edges) in {ocean_path} in {time.perf_counter() - t_l:.2f}s")
            on_land = None
            if land_images is not None:
                # the images that hold only land (reference src/utils.py:46-69, mark_land_images), over the image list --evaluate-kfold
                # makes its table of: the source's listing, or with --tile-scenes the list --evaluate-kfold-images gives
                from . import evaluate as aqeval, land_images as aqli
                t_i = time.perf_counter()
                swept_li = None
                if not tile_scenes:
                    from .dataloader import list_images
                    swept_li = sorted({aqeval._stem(f_) for f_ in list_images(source)})
                li_out = land_images or str(save_dir / aqli.CSV_FILE)
                li = aqli.land_images_from_names(aqeval.land_image_names(table, None, evaluate_kfold_images, swept_li), geocode_bboxes, segs, li_out,
                                                 land_images_indent)
                on_land = [s_ for s_, l_ in zip(li["stems"], li["on_land"]) if l_]
                log(f"{aqli.describe(li)} in {li_out} in {time.perf_counter() - t_i:.2f}s")
            dd = None
            hw = None
            if facilities is not None or tonnage is not None or dedup_years is not None or model_errors is not None:
                # An image this rank's sweep did not see (another rank's, or one a resumed run had finished) counts as the 1024-px tile the
                # geocoding assumes anyway.
                hw = np.asarray([image_hw.get(str(s_), (geocode.IM_HEIGHT, geocode.IM_WIDTH)) for s_ in table["stems"]], np.int64).reshape(-1, 2)
            if dedup_years is not None:
                # the step before every clustering by pass (reference src/utils_tonnage.py:668-911, :979-995), on the key and the outlines
                # this sweep has just written; detections.geojson stays as it is and cage_ids stay its row numbers
                from . import dedup as aqdedup
                t_d = time.perf_counter()
                dd_out = dedup_years or str(save_dir)
                dd = aqdedup.dedup_from_table(table, key_out, geom_out, dd_out, dedup_selection, dedup_seed, facilities_conf, ocean,
                                              hw[table["image"], 1], hw[table["image"], 0])
                log(f"dedup years: {aqdedup.describe(dd)} in {dd_out} in {time.perf_counter() - t_d:.2f}s")
            bathy = None
            if bathymetry:
                # the depth raster under the cages (reference src/utils_tonnage.py:591-665), read once for both steps below
                from . import bathymetry as aqbathy
                t_b = time.perf_counter()
                bathy = aqbathy.settings([bathymetry] if isinstance(bathymetry, str) else list(bathymetry), table, ocean, bathymetry_statistic,
                                         tonnage_default_depth, tonnage_min_depth)
                log(f"bathymetry: a window of {bathy['grid']['data'].shape[0]} x {bathy['grid']['data'].shape[1]} cells of "
                    f"{', '.join(os.path.basename(f_) for f_ in bathy['grid']['files'])} in {time.perf_counter() - t_b:.2f}s")
            if facilities is not None:
                # the steps after it (reference src/process_yolo/calc_net_areas.py, src/cluster_facilities.py)
                from . import facilities as aqfac
                t_f = time.perf_counter()
                fac_out = facilities or str(save_dir / "facilities.geojson")
                fac = aqfac.facilities_from_table(table, fac_out, facilities_by, facilities_conf, facilities_eps, facilities_min_cages,
                                                  hw[table["image"], 1], hw[table["image"], 0], keep=ocean, bathymetry=bathy, dedup=dd)
                log(f"{len(fac['facility_index'])} facilities of {int((fac['_members'] >= 0).sum())} cages in {fac_out} "
                    f"in {time.perf_counter() - t_f:.2f}s")
                if facility_sites is not None:
                    # known against additional facilities (reference src/Results/FacilitiesMaps.py:64-188) on the table just made
                    from . import facility_sites as aqsites
                    t_s = time.perf_counter()
                    fs_out = facility_sites_out or str(save_dir)
                    fs_res = aqsites.facility_sites_from_table(fac, table, facility_sites, geocode_bboxes, fs_out, facility_sites_truth)
                    log(f"{aqsites.describe(fs_res)} in {fs_out} in {time.perf_counter() - t_s:.2f}s")
            if evaluate is not None:
                # the reference's tuning step (src/get_kfold_cluster_performance.py) on the same table, the ocean rows when there are any
                from . import evaluate as aqeval
                t_e = time.perf_counter()
                grids = aqeval.grids_from_options(evaluate_conf, evaluate_eps, evaluate_min_cages)
                ev_out = evaluate_out or str(save_dir)
                ev = aqeval.evaluate_table(table, evaluate, ev_out, *grids, op=(facilities_conf, facilities_eps, facilities_min_cages), keep=ocean,
                                           images=aqeval.read_image_list(evaluate_images) if evaluate_images else None,
                                           dedup_overlaps=geocode_bboxes if dedup_overlaps is not None else None)
                log(f"{aqeval.describe(ev)} in {ev_out} in {time.perf_counter() - t_e:.2f}s")
                if evaluate_kfold is not None:
                    # the rest of that script: the image table (every image of the sweep, with or without a detection: the source's
                    # listing, the same on every rank; with --tile-scenes the list --evaluate-kfold-images gives, which run() insists on),
                    # the hold-out, the stratified folds, the grid per fold and the winners on the test images, all folds in one call per
                    # distance
                    from . import kfold as aqkfold
                    t_k = time.perf_counter()
                    swept = None
                    if not tile_scenes:
                        from .dataloader import list_images
                        swept = sorted({aqeval._stem(f_) for f_ in list_images(source)})
                    kf = aqeval.kfold_from_options(table, evaluate, ev_out, grids, (facilities_conf, facilities_eps, facilities_min_cages), ocean,
                                                   aqeval.read_image_list(evaluate_images) if evaluate_images else None, evaluate_kfold,
                                                   evaluate_kfold_images, evaluate_known_sites, evaluate_kfold_seed, evaluate_kfold_test,
                                                   geocode_bboxes, names=swept, dedup_overlaps=geocode_bboxes if dedup_overlaps is not None else None,
                                                   land=on_land)
                    log(f"{aqkfold.describe(kf)} in {ev_out} in {time.perf_counter() - t_k:.2f}s")
                if performance is not None:
                    # the accuracy section (reference src/Results/ModelPerformance.py, get_bucket_info_table, upper_bound_calculation.R) on
                    # the same table and labels: the detections before any land step, the image list of --land-images and --evaluate-kfold
                    from . import performance as aqperf
                    t_p = time.perf_counter()
                    swept_p = None
                    if not tile_scenes:
                        from .dataloader import list_images
                        swept_p = sorted({aqeval._stem(f_) for f_ in list_images(source)})
                    pf_out = performance or str(save_dir)
                    pf = aqperf.performance_from_options(table, evaluate, pf_out, geocode_bboxes, names=swept_p, kfold_images=evaluate_kfold_images,
                                                         sample_file=performance_sample, known_sites=evaluate_known_sites, land=on_land, keep=unique,
                                                         dedup_overlaps=geocode_bboxes if dedup_overlaps is not None else None, **performance_settings)
                    log(f"{aqperf.describe(pf)} in {pf_out} in {time.perf_counter() - t_p:.2f}s")
            computed_errors = None
            if model_errors is not None:
                # the model's cage-area error per pass and type (reference src/utils_tonnage.py:130-203) from the same table and the labels
                # --evaluate reads, the ocean rows when there are any; what the bootstrap below then draws its model errors from
                from . import model_errors as aqerr
                t_m = time.perf_counter()
                me_out = model_errors_out or str(save_dir)
                me = aqerr.model_errors_from_table(table, model_errors, me_out, facilities_conf if model_errors_conf is None else model_errors_conf,
                                                   keep=ocean, widths=hw[table["image"], 1], heights=hw[table["image"], 0],
                                                   dedup_overlaps=geocode_bboxes if dedup_overlaps is not None else None)
                computed_errors = me["errors"]
                log(f"{aqerr.describe(me)} in {me_out} in {time.perf_counter() - t_m:.2f}s")
            if tonnage is not None:
                # the reference's measuring step (src/utils_tonnage.py): facilities per image pass whatever --facilities-by says (the
                # facility file above stays as it is), the ocean rows when there are any
                from . import tonnage as aqton
                from . import missing as aqmiss
                t_t = time.perf_counter()
                ton_out = tonnage or str(save_dir)
                est = aqton.tonnage_from_table(table, ton_out, tonnage_factors, tonnage_errors, tonnage_depths, tonnage_K, tonnage_seed, tonnage_mix,
                                               tonnage_min_depth, tonnage_default_depth, facilities_conf, facilities_eps, facilities_min_cages,
                                               hw[table["image"], 1], hw[table["image"], 0], keep=ocean, bathymetry=bathy, dedup=dd,
                                               **({"errors": computed_errors} if computed_errors is not None else {}),
                                               **({"missing": aqmiss.settings(tonnage_missing, key_out, geom_out, geocode_bboxes)}
                                                  if tonnage_missing is not None else {}),
                                               **({"near_sites": tonnage_near_sites} if tonnage_near_sites else {}))
                log(f"tonnage: {aqton.describe(est)} in {ton_out} in {time.perf_counter() - t_t:.2f}s")
    manifest.close()
    eng.close()
    return save_dir


def _calibration_tiles(source, tile_scenes, imgsz, stride, dev, n=16):
    """Up to `n` letterboxed tiles sampled evenly over the sweep's sorted file list (not its first files, which all come from one scene):
    uint8 CUDA [b, H, W, 3], every tile of the first sample's original size.  Host decode -- it runs once per sweep."""
    from .engine import letterbox_device
    if tile_scenes:
        from .scenes import list_scenes, read_scene, tile_grid
        scenes = list_scenes(source)
        picks = []
        for sp in scenes[:: max(1, len(scenes) // 4)][:4]:
            arr = read_scene(sp)
            grid = tile_grid(arr.shape[1], arr.shape[0], int(tile_scenes))
            grid = [g for g in grid if (g[2], g[3]) == (int(tile_scenes), int(tile_scenes))] or grid     # (scenes smaller than one tile: edge tiles)
            for x, y, w, h in grid[:: max(1, len(grid) // 4)][:4]:
                picks.append(np.ascontiguousarray(arr[y:y + h, x:x + w, :3]))
    else:
        from .dataloader import list_images, read_rgb
        files = list_images(source)
        picks = [read_rgb(f) for f in files[:: max(1, len(files) // n)][:n]]
    picks = [p for p in picks if p.shape == picks[0].shape]
    if not picks:
        raise ValueError("fp8 calibration: no tiles to calibrate on")
    return letterbox_device(torch.from_numpy(np.stack(picks)).to(dev), tuple(imgsz), stride, True)


def main(argv: Optional[List[str]] = None) -> int:
    opt = parse_opt(argv)
    run(**vars(opt))
    return 0


if __name__ == "__main__":
    sys.exit(main())
