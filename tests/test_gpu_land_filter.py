"""--land-filter on the GPU: aq_land_filter_f64 (csrc/land_filter.hip) through engine.land_flags / land.land_flags against the hand-written
flags and the numpy restatement, byte for byte.  The cases and their expected bytes are those of tests/test_land_filter.py.  The
command-line step and the detect.py sweep each run in a child process under their own time limit."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_land_filter import (NAMED, TOUCH, TOUCH_LAND, comb_case, label_run, named_boxes, named_expected, named_land, no_near_ties, random_case,
                              touch_boxes, touch_expected)

from aquaculture_amd import land

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gpu_flags(boxes, segs, band_height=None, times=None):
    from aquaculture_amd.engine import land_flags
    out = land_flags(torch.from_numpy(np.ascontiguousarray(boxes)).cuda(), torch.from_numpy(np.ascontiguousarray(segs)).cuda(), band_height, times=times)
    assert out.dtype == torch.uint8 and out.is_cuda and out.shape == (boxes.shape[0],)
    return out.cpu().numpy()


def test_named_cases_both_bits(lib):
    for bh in (None, 1000.0, 0.37):                         # the default, one band, bands thinner than the sliver is wide
        got = gpu_flags(named_boxes(), named_land(), bh)
        assert got.tolist() == named_expected().tolist(), (bh, dict(zip(sorted(NAMED), got.tolist())))


def test_exact_touches_count_as_on_land(lib):
    for bh in (None, 1.0, 0.5, 100.0):                      # band edges on the touched coordinates, and away from them
        got = gpu_flags(touch_boxes(), TOUCH_LAND, bh)
        assert got.tolist() == touch_expected().tolist(), (bh, dict(zip(sorted(TOUCH), got.tolist())))
    point = np.asarray([[4.0, 4.0, 4.0, 4.0]])
    assert gpu_flags(np.asarray([[4.0, 4, 6, 6], [2.0, 2, 5, 5], [5.0, 5, 7, 7]]), point).tolist() == [1, 1, 0]


def test_random_case_is_the_numpy_restatement_at_every_band_height(lib):
    """4,000 wavefronts, 1,000 workgroups; 1 band, 7 bands, the default and 4096 bands."""
    boxes, segs, _ = random_case()
    assert no_near_ties(boxes, segs)
    want = land.land_flags_numpy(boxes, segs)
    extent = float(max(segs[:, 1].max(), segs[:, 3].max()) - min(segs[:, 1].min(), segs[:, 3].min()))
    seen = []
    for bh, bands in ((2.0 * extent, 1), (extent / 6.5, 7), (None, None), (extent / 4095.5, 4096)):
        t = {}
        got = gpu_flags(boxes, segs, bh, times=t)
        assert bands is None or t["nbands"] == bands, t
        assert t["entries"] >= 400 and t["kernel_ms"] > 0 and t["table_ms"] > 0
        assert np.array_equal(got, want), (bh, np.nonzero(got != want)[0][:10])
        seen.append(t["nbands"])
    assert len(set(seen)) == 4, seen                        # four different tables, the same bytes
    assert np.array_equal(land.land_flags(boxes, segs), want)


def test_one_segment_in_every_band(lib):
    segs, boxes = comb_case()
    want = land.land_flags_numpy(boxes, segs)
    assert (np.bincount(want, minlength=4) >= 20).all(), np.bincount(want, minlength=4)
    for bh in (None, 7.3, 3000.0 / 4095.5, 1e4):
        t = {}
        got = gpu_flags(boxes, segs, bh, times=t)
        assert t["entries"] >= t["nbands"] + 300             # the long segment is entered in every band
        assert np.array_equal(got, want), (bh, np.nonzero(got != want)[0][:10])


def test_the_same_bytes_twice(lib):
    from aquaculture_amd.engine import land_flags
    boxes, segs, _ = random_case()
    b, s = torch.from_numpy(boxes).cuda(), torch.from_numpy(segs).cuda()
    assert torch.equal(land_flags(b, s), land_flags(b, s))


def test_no_boxes_and_no_land(lib):
    boxes, segs, _ = random_case()
    assert gpu_flags(np.zeros((0, 4)), segs).shape == (0,)
    assert gpu_flags(boxes[:100], np.zeros((0, 4))).tolist() == [0] * 100
    assert gpu_flags(np.zeros((0, 4)), np.zeros((0, 4))).shape == (0,)
    assert land.land_flags(np.zeros((0, 4)), segs).shape == (0,)


def test_bad_arguments_are_refused_and_nothing_is_launched(lib):
    from aquaculture_amd import engine
    boxes, segs = named_boxes(), named_land()
    N, E = boxes.shape[0], segs.shape[0]
    b, s = torch.from_numpy(boxes).cuda(), torch.from_numpy(segs).cuda()
    entry_seg, band_start, nbands, Y0, h = engine.land_band_table(s)
    entries = entry_seg.shape[0]
    need = int(lib.aq_land_scratch_bytes(entries))
    assert need == 32 * entries
    scratch = torch.full((need + 32,), 0x5A, dtype=torch.uint8, device="cuda")
    flags = torch.full((N,), 0x77, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def call(seg_p=s.data_ptr(), E_=E, entry_p=entry_seg.data_ptr(), entries_=entries, start_p=band_start.data_ptr(), nbands_=nbands, Y0_=Y0, h_=h,
             boxes_p=b.data_ptr(), N_=N, scratch_p=scratch.data_ptr(), scratch_bytes=need, flags_p=flags.data_ptr()):
        return lib.aq_land_filter_f64(seg_p, E_, entry_p, entries_, start_p, nbands_, Y0_, h_, boxes_p, N_, scratch_p, scratch_bytes, flags_p, stream)

    for kw, msg in (({"h_": 0.0}, "band height"), ({"h_": -1.0}, "band height"), ({"h_": float("nan")}, "band height"), ({"h_": float("inf")}, "band height"),
                    ({"Y0_": float("nan")}, "Y0"), ({"Y0_": float("-inf")}, "Y0"), ({"nbands_": 0}, "nbands"),
                    ({"seg_p": None}, "null pointer"), ({"entry_p": None}, "null pointer"), ({"start_p": None}, "null pointer"),
                    ({"boxes_p": None}, "null pointer"), ({"scratch_p": None}, "null pointer"), ({"flags_p": None}, "null pointer"),
                    ({"seg_p": s.data_ptr() + 8}, "unaligned"), ({"boxes_p": b.data_ptr() + 16}, "unaligned"), ({"scratch_p": scratch.data_ptr() + 8}, "unaligned"),
                    ({"entry_p": entry_seg.data_ptr() + 2}, "unaligned"),
                    ({"E_": 1 << 31}, "2\\^31"), ({"N_": 1 << 31}, "2\\^31"), ({"entries_": 1 << 31}, "2\\^31"), ({"E_": -1}, "2\\^31"),
                    ({"scratch_bytes": need - 1}, "scratch")):
        assert call(**kw) == -1, kw
        assert re.search(msg, lib.aq_last_error().decode()), (kw, lib.aq_last_error())
        torch.cuda.synchronize()
        assert bool((flags == 0x77).all()) and bool((scratch == 0x5A).all()), kw
    # N = 0 does nothing, whatever the pointers; E = 0 zeroes the flags and needs no table
    assert lib.aq_land_filter_f64(None, E, None, entries, None, nbands, Y0, h, None, 0, None, 0, None, stream) == 0
    torch.cuda.synchronize()
    assert bool((flags == 0x77).all())
    with pytest.raises(ValueError, match="band height"):
        engine.land_flags(b, s, 0.0)
    with pytest.raises(ValueError, match=r"\d{10,} band entries"):
        engine.land_flags(b, s, 1e-9)
    torch.cuda.synchronize()
    assert bool((flags == 0x77).all()) and bool((scratch == 0x5A).all())
    assert call() == 0                                      # and the same arguments, all valid, run
    torch.cuda.synchronize()
    assert flags.cpu().tolist() == named_expected().tolist() and bool((scratch[need:] == 0x5A).all())
    assert lib.aq_land_filter_f64(None, 0, None, 0, None, 1, 0.0, 1.0, None, N, None, 0, flags.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    assert bool((flags == 0).all())


# ---- python -m aquaculture_amd.land ----

def test_command_line_gpu_and_cpu_write_the_same_file(lib, tmp_path):
    labels, csv_path, land_path = label_run(tmp_path)
    outs = []
    for extra in ([], ["--cpu"]):
        out = str(tmp_path / ("ocean" + "".join(extra) + ".geojson"))
        r = subprocess.run(["timeout", "-k", "10", "150", sys.executable, "-m", "aquaculture_amd.land", "--labels", labels, "--geocode-bboxes", csv_path,
                            "--land", land_path, "--out", out, *extra], cwd=ROOT, capture_output=True, text=True, timeout=180)
        assert r.returncode == 0, r.stderr[-3000:]
        assert re.search(r"15 of 34 detections at sea \(7 land edges\)", r.stdout), r.stdout
        outs.append(open(out).read())
    assert outs[0] == outs[1] and outs[0].count('"index"') == 15


# ---- detect.py --land-filter ----

def test_detect_py_writes_the_ocean_detections_and_clusters_them(lib, tmp_path):
    """An engine sweep over four synthetic 640-px tiles with the synthetic checkpoint, geocoded, filtered and clustered in the same run: the
    ocean file and the facilities equal what the host restatements make of the run's label files; detections.geojson is what it is without
    the flag."""
    import json
    from PIL import Image
    from test_gpu_facilities import synthetic_run
    from test_land_filter import lonlat_ring
    from aquaculture_amd import checkpoint, facilities, geocode, tiles
    (tmp_path / "jpegs").mkdir()
    for k, i in enumerate((0, 3, 19, 20)):
        Image.fromarray(tiles.synthetic_tile(i, 640)).save(tmp_path / "jpegs" / f"ORTHOIMAGERY.ORTHOPHOTOS{2015 - k % 2}_3_{1024 * k}_0.jpeg", quality=95)
    checkpoint.write_synthetic_checkpoint(str(tmp_path / "synth.pt"), "yolov5m", 5)
    _, csv_path = synthetic_run(tmp_path)
    x0, y0 = (float(v) for v in geocode.lonlat_to_mercator(np.float64(3.5), np.float64(43.3)))
    west = [(x0 - 50, y0 - 50), (x0 + 400, y0 - 50), (x0 + 500, y0 + 1900), (x0 - 50, y0 + 1900)]      # the scene's western quarter is land
    land_path = tmp_path / "land.geojson"
    land_path.write_text(json.dumps({"type": "Polygon", "coordinates": [lonlat_ring(west)]}))
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "yolov5", "detect.py"), "--weights", str(tmp_path / "synth.pt"),
                        "--source", str(tmp_path / "jpegs"), "--save-txt", "--save-conf", "--nosave", "--project", str(tmp_path / "runs"), "--name", "land",
                        "--batch-size", "4", "--geocode-bboxes", csv_path, "--land-filter", str(land_path), "--facilities", "--facilities-conf", "0.25",
                        "--facilities-eps", "25", "--facilities-min-cages", "4", "--facilities-by", "pass"], capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    run = tmp_path / "runs" / "land"
    print(" ".join(l for l in (r.stdout + r.stderr).splitlines() if "at sea" in l or "facilities of" in l))
    assert "land_filter" not in json.load(open(run / "run_params.json"))
    table = geocode.geocode_label_dir(str(run / "labels"), csv_path, str(tmp_path / "want_detections.geojson"))
    assert open(run / "detections.geojson").read() == open(tmp_path / "want_detections.geojson").read()
    keep = land.ocean_rows(table, land.load_land_geojson(str(land_path)), cpu=True)
    assert 50 <= keep.sum() <= keep.shape[0] - 50
    assert f"{int(keep.sum())} of {keep.shape[0]} detections at sea (4 land edges)" in r.stdout + r.stderr
    land.write_ocean_geojson(str(tmp_path / "want_ocean.geojson"), table["stems"], table, keep)
    assert open(run / "ocean_detections.geojson").read() == open(tmp_path / "want_ocean.geojson").read()
    want_out = str(tmp_path / "want.geojson")
    fac = facilities.facilities_from_table(table, want_out, "pass", 0.25, 25.0, 4, 640, 640, cpu=True, keep=keep)
    assert len(fac["facility_index"]) >= 1 and not any(set(ids) - set(np.nonzero(keep)[0].tolist()) for ids in fac["cage_ids"])
    assert json.load(open(run / "facilities.geojson")) == json.load(open(want_out))
    assert json.load(open(run / "facilities_detections.geojson")) == json.load(open(facilities.detections_path(want_out)))
