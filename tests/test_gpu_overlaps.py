"""--dedup-overlaps on the GPU: csrc/overlaps.hip through engine.overlap_partners / engine.overlap_clip gives the bytes of
overlaps.partners_numpy / overlaps.clip_numpy on the named cases and the random case of tests/test_overlaps.py, through one band, a few,
the default and many; with more than 64 partners; without boxes or detections; at detection counts around a workgroup's four wavefronts;
nothing depends on bytes the kernels do not own and nothing is written beside the outputs; the launchers refuse by their arguments alone;
both command lines write the --cpu route's files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from poison import poisoned
from test_overlaps import NAMED, named_arrays, named_expected, overlap_run, random_case, same_bytes, strips_case

from aquaculture_amd import engine, overlaps

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gpu_partners(boxes, nbands=None):
    start, partner = overlaps.partners_gpu(boxes, nbands)
    want_start, want_partner = overlaps.partners_numpy(boxes)
    assert start.dtype == want_start.dtype == np.int64 and partner.dtype == want_partner.dtype == np.int32
    assert start.tobytes() == want_start.tobytes() and partner.tobytes() == want_partner.tobytes(), nbands
    return start, partner


def gpu_clip(boxes, det_row, dets, nbands=None):
    """Partner lists and clip from the GPU, both against the host's, byte for byte."""
    start, partner = gpu_partners(boxes, nbands)
    got = overlaps.clip_gpu(boxes, start, partner, det_row, dets)
    same_bytes(got, overlaps.clip_numpy(boxes, start, partner, det_row, dets))
    return got


@pytest.mark.parametrize("name", list(NAMED))
def test_named_cases_are_the_restatements_bytes(lib, name):
    boxes, det_row, dets = named_arrays(name)
    for nbands in (None, 1, 3):
        same_bytes(gpu_clip(boxes, det_row, dets, nbands), named_expected(name))


def test_random_case_and_the_bands(lib):
    boxes, det_row, dets, literal = random_case()
    for nbands in (1, 5, None, 4000):                       # one band, a handful, the default, many more bands than boxes
        gpu_partners(boxes, nbands)
    same_bytes(gpu_clip(boxes, det_row, dets), literal)
    for m in (1, 3, 4, 5, 7):                               # a workgroup holds four detections
        got = gpu_clip(boxes, det_row[100:100 + m], dets[100:100 + m])
        for k in ("state", "clip_bounds", "clip_area"):
            assert got[k].tobytes() == literal[k][100:100 + m].tobytes()


def test_more_than_64_partners(lib):
    boxes, det_row, dets, want = strips_case()
    for nbands in (None, 1, 300):
        start, partner = gpu_partners(boxes, nbands)
    assert start[-1] - start[-2] == 70
    got = gpu_clip(boxes, det_row, dets)
    assert got["state"].tolist() == want.tolist() and got["clip_area"][0] == 1420.0 and got["has_region"].tolist() == [1] * 71


def test_no_boxes_and_no_detections(lib):
    none = np.zeros((0, 4))
    start, partner = gpu_partners(none)
    assert start.tolist() == [0] and partner.shape == (0,)
    got = overlaps.clip_gpu(none, start, partner, np.zeros(0, np.int32), none)
    assert [got[k].shape for k in ("state", "clip_bounds", "clip_area", "has_region")] == [(0,), (0, 4), (0,), (0,)]
    boxes = named_arrays("straddling an L")[0]
    got = gpu_clip(boxes, np.zeros(0, np.int32), none)
    assert got["state"].shape == (0,) and got["has_region"].tolist() == [1, 1]


def test_nothing_depends_on_unowned_bytes_and_nothing_else_is_written(lib, monkeypatch):
    """Every input sits in a poisoned allocation with a guard behind it, as do the outputs the wrappers allocate: the same bytes under both
    fills, equal to the host's, and every guard intact."""
    boxes, det_row, dets, literal = random_case()
    t = overlaps.band_table(boxes)
    want_start, want_partner = overlaps.partners_numpy(boxes)
    outs = {}
    for byte in (0x00, 0xFF):
        with poisoned(monkeypatch, byte) as p:
            def dev(a):
                a = np.ascontiguousarray(a)
                d = torch.empty(a.shape, dtype=torch.from_numpy(a).dtype, device="cuda")
                d.copy_(torch.from_numpy(a))
                return d
            start, partner = engine.overlap_partners(dev(boxes), dev(t["entry_box"]), dev(t["band_start"]), t["nbands"], t["Y0"], t["h"])
            res = engine.overlap_clip(dev(boxes), start, partner, dev(det_row), dev(dets))
            torch.cuda.synchronize()
            outs[byte] = [v.cpu().numpy().copy() for v in (start, partner, *res)]
            p.check_guards()
            assert not p.passed_through, p.passed_through
    for a, b in zip(outs[0x00], outs[0xFF]):
        assert a.tobytes() == b.tobytes()
    assert outs[0][0].tobytes() == want_start.tobytes() and outs[0][1].tobytes() == want_partner.tobytes()
    same_bytes(dict(zip(("state", "clip_bounds", "clip_area", "has_region"), outs[0][2:])), literal)


def test_launchers_refuse_by_their_arguments(lib):
    stream = torch.cuda.current_stream().cuda_stream
    z = lambda n, dt: torch.zeros(n, dtype=dt, device="cuda")
    boxes, start, entry, bs = z((4, 4), torch.float64), z(5, torch.int64), z(4, torch.int32), z(2, torch.int32)
    base = dict(boxes=boxes.data_ptr(), n=4, entry=entry.data_ptr(), entries=4, bs=bs.data_ptr(), nbands=1, Y0=0.0, h=1.0, start=start.data_ptr(),
                partner=None, cap=0)
    call = lambda **kw: lib.aq_overlap_partners_f64(*{**base, **kw}.values(), stream)
    assert call() == 0
    for kw, text in (({"n": 1 << 31}, "boxes"), ({"entries": -1}, "band entries"), ({"nbands": 0}, "nbands"), ({"nbands": (1 << 31) - 1}, "nbands"),
                     ({"h": 0.0}, "band height"), ({"h": float("nan")}, "band height"), ({"Y0": float("inf")}, "Y0"), ({"start": None}, "start"),
                     ({"boxes": None}, "null pointer"), ({"boxes": boxes.data_ptr() + 8}, "unaligned"), ({"cap": 1 << 31}, "partners")):
        assert call(**kw) != 0
        msg = lib.aq_last_error()
        assert msg.startswith(b"overlaps:") and text.encode() in msg, (kw, msg)
    has = z(4, torch.uint8)
    clip = lambda n, m, T=0, boxes_p=boxes.data_ptr(): lib.aq_overlap_clip_f64(boxes_p, n, start.data_ptr(), None, T, None, None, m, None, None, None,
                                                                                 has.data_ptr(), stream)
    assert clip(0, 0) == 0 and clip(4, 0) == 0
    for args in ((1 << 31, 0), (4, -1), (4, 0, 1 << 31), (4, 1), (4, 0, 0, None)):
        assert clip(*args) != 0 and lib.aq_last_error().startswith(b"overlaps:")
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="overlaps: dets has to be a contiguous CUDA"):
        engine.overlap_clip(boxes, start, z(0, torch.int32), z(2, torch.int32), z((2, 4), torch.float32))
    with pytest.raises(ValueError, match="overlaps: band_start"):
        engine.overlap_partners(boxes, entry, bs, 2, 0.0, 1.0)


# ---- the command lines ----

def _same_files(got_dir, want_dir):
    for name in (overlaps.DETECTIONS_FILE, overlaps.REGIONS_FILE):
        assert open(os.path.join(got_dir, name), "rb").read() == open(os.path.join(want_dir, name), "rb").read(), name
    got, want = (json.load(open(os.path.join(d, overlaps.SUMMARY_FILE))) for d in (got_dir, want_dir))
    assert (got.pop("device"), want.pop("device")) == ("gpu", "cpu") and {"partners_ms", "clip_ms"} <= set(got.pop("times")) and want.pop("times")
    assert got == want                                      # (the device and the times are what the two routes may differ in)
    return got


def test_command_line_gpu_and_cpu_write_the_same_files(lib, tmp_path):
    labels, csv_path = overlap_run(tmp_path)
    for extra in ([], ["--cpu"]):
        r = subprocess.run(["timeout", "-k", "10", "150", sys.executable, "-m", "aquaculture_amd.overlaps", "--labels", labels, "--geocode-bboxes", csv_path,
                            "--out", str(tmp_path / ("out" + "".join(extra))), *extra], cwd=ROOT, capture_output=True, text=True, timeout=180)
        assert r.returncode == 0, r.stderr[-3000:]
        assert "10 of 14 detections kept (9 whole, 1 clipped, 0 touching, 4 dropped); 0 of 2 boxes have no region" in r.stdout, r.stdout
    assert _same_files(str(tmp_path / "out"), str(tmp_path / "out--cpu"))["states"]["clipped"] == 1


def test_detect_py_counts_every_cage_once(lib, tmp_path):
    """An engine sweep over four synthetic 640-px tiles of scene 3 with the synthetic checkpoint; an earlier box of the file covers the
    scene's western 350 m: the three files equal what the host route makes of the run's label files, the facilities are those of the
    survivors, detections.geojson is what it is without the flag."""
    from PIL import Image
    from aquaculture_amd import checkpoint, facilities, geocode, tiles
    (tmp_path / "jpegs").mkdir()
    for k, i in enumerate((0, 3, 19, 20)):
        Image.fromarray(tiles.synthetic_tile(i, 640)).save(tmp_path / "jpegs" / f"ORTHOIMAGERY.ORTHOPHOTOS{2015 - k % 2}_3_{1024 * k}_0.jpeg", quality=95)
    checkpoint.write_synthetic_checkpoint(str(tmp_path / "synth.pt"), "yolov5m", 5)
    x0, y0 = (float(v) for v in geocode.lonlat_to_mercator(np.float64(3.5), np.float64(43.3)))
    csv_path = str(tmp_path / "wanted_bboxes.csv")
    with open(csv_path, "w") as f:
        f.write(",geometry\n")
        for ind, a, c in ((1, x0 - 1493.2, x0 + 350.0), (3, x0, x0 + 1843.2)):
            b, d = y0, y0 + 1843.2
            f.write(f'{ind},"POLYGON (({c!r} {b!r}, {c!r} {d!r}, {a!r} {d!r}, {a!r} {b!r}, {c!r} {b!r}))"\n')
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "yolov5", "detect.py"), "--weights", str(tmp_path / "synth.pt"),
                        "--source", str(tmp_path / "jpegs"), "--save-txt", "--save-conf", "--nosave", "--project", str(tmp_path / "runs"), "--name", "over",
                        "--batch-size", "4", "--geocode-bboxes", csv_path, "--dedup-overlaps", "--facilities", "--facilities-conf", "0.25",
                        "--facilities-eps", "25", "--facilities-min-cages", "4", "--facilities-by", "pass"], capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    run = tmp_path / "runs" / "over"
    print(" ".join(l for l in (r.stdout + r.stderr).splitlines() if "dedup overlaps" in l or "facilities of" in l))
    assert "dedup_overlaps" not in json.load(open(run / "run_params.json"))
    table = geocode.geocode_label_dir(str(run / "labels"), csv_path, str(tmp_path / "want_detections.geojson"))
    assert open(run / "detections.geojson", "rb").read() == open(tmp_path / "want_detections.geojson", "rb").read()
    want = overlaps.dedup_from_table(table, csv_path, str(tmp_path / "want"), cpu=True)
    s = _same_files(str(run), str(tmp_path / "want"))
    assert s["states"]["dropped"] >= 20 and s["states"]["whole"] >= 50 and f"dedup overlaps: {overlaps.describe(s)}" in r.stdout + r.stderr
    fac = facilities.facilities_from_table(table, str(tmp_path / "want.geojson"), "pass", 0.25, 25.0, 4, 640, 640, cpu=True, keep=want["keep"])
    assert not any(set(ids) - set(np.nonzero(want["keep"])[0].tolist()) for ids in fac["cage_ids"])
    assert json.load(open(run / "facilities.geojson")) == json.load(open(tmp_path / "want.geojson"))
