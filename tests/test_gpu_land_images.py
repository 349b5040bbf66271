"""--land-images on the GPU: aq_land_images_f64 (csrc/land_images.hip) through engine.land_images against the numpy restatement, flags and
dist2 bit for bit, at every band height; the hand-decided cases of tests/test_land_images.py; the outputs inside poisoned, guarded
buffers; the refusals.  The command-line step runs in a child process under its own time limit."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from poison import poisoned
from test_land_filter import OX, OY, label_run, ring_segments
from test_land_images import CAP2, HAND, R, all_images, check_hand, hand_case, star_case

from aquaculture_amd import land_images as li

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gpu(rects, segs, indent=R, band_height=None, times=None):
    from aquaculture_amd.engine import land_images
    rects, segs = np.ascontiguousarray(rects, np.float64).reshape(-1, 4), np.ascontiguousarray(segs, np.float64).reshape(-1, 4)
    f, d = land_images(torch.from_numpy(rects).cuda(), torch.from_numpy(segs).cuda(), indent, band_height, times=times)
    assert f.dtype == torch.uint8 and d.dtype == torch.float64 and f.is_cuda and d.is_cuda and f.shape == d.shape == (rects.shape[0],)
    return f.cpu().numpy(), d.cpu().numpy()


def same(got, want, what):
    """flags equal and dist2 equal as bit patterns"""
    assert np.array_equal(got[0], want[0]), (what, np.nonzero(got[0] != want[0])[0][:10])
    assert np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64)), (what, np.nonzero(got[1] != want[1])[0][:10])


def test_cases_decided_by_hand_at_three_band_heights(lib):
    for name in sorted(HAND):
        rects, segs = hand_case(name)
        want = li.land_images_numpy(rects, segs, R)
        for bh in (None, 0.5, 7.0):                         # the default; thinner than the indent (the nearest edge and the parity run are in different bands); 7 m
            got = gpu(rects, segs, R, bh)
            check_hand(name, *got)
            same(got, want, (name, bh))


def test_random_case_is_the_restatement_at_every_band_height_inside_poisoned_buffers(lib, monkeypatch):
    """1,500 wavefronts over 400 edges; bands of 0.5 m, 7 m, the default and one band: four tables, the same bytes and the same doubles, and
    no byte outside the [N] bytes and [N] doubles (nor outside the scratch) is written."""
    rects, segs = star_case()
    want = li.land_images_numpy(rects, segs, R)
    extent = float(max(segs[:, 1].max(), segs[:, 3].max()) - min(segs[:, 1].min(), segs[:, 3].min()))
    seen = []
    for bh in (0.5, 7.0, None, 2.0 * extent):
        for byte in (0xFF, 0x00):
            with poisoned(monkeypatch, byte) as p:
                t = {}
                got = gpu(rects, segs, R, bh, times=t)
                torch.cuda.synchronize()
                p.check_guards()
                assert p.intercepted >= 3                   # the flags, the distances, the scratch
            assert t["entries"] >= 400 and t["kernel_ms"] > 0 and t["table_ms"] > 0
            same(got, want, (bh, byte))
        seen.append(t["nbands"])
    assert len(set(seen)) == 4 and seen[-1] == 1, seen
    same(li.land_images_gpu(rects, segs, R), want, "host arrays in, host arrays out")
    mark, flags, dist2 = li.on_land(rects, segs, R)
    assert np.array_equal(mark, want[0] == 2) and np.array_equal(dist2, want[1])
    same(gpu(rects, segs, 12.5), li.land_images_numpy(rects, segs, 12.5), "another indent")


@pytest.mark.parametrize("E", [63, 64, 65, 129])
def test_run_lengths_around_the_waves_stride_and_rectangle_counts_around_the_block(lib, E):
    """One band, so the run of every rectangle is all E entries; 1, 4 and 5 rectangles (four waves to a block).  The nearest edge is the
    last entry for the first rectangle, the first entry for the second."""
    a = np.arange(E) * (2 * np.pi / E)
    ring = np.round(np.stack([OX + 60 * np.cos(a), OY + 60 * np.sin(a)], 1) * 8) / 8
    segs = ring_segments(ring)                              # the edge from vertex 0 (at angle 0) upwards is the first entry, the one up to it the last
    rects = np.asarray([[62.0, -14.0, 70, -1], [62.5, 1, 70, 14], [-10, -10, 10, 10], [-3, 52, 3, 57], [-80, -80, -70, -70]]) + [OX, OY, OX, OY]
    want = li.land_images_numpy(rects, segs, R)
    assert want[0].tolist()[2] == 2 and want[0].tolist()[4] == 0 and want[1][4] == CAP2 and 0 < want[1][0] < 25 and 0 < want[1][1] < 25
    d_last = li.land_images_numpy(rects[:1], segs[-1:], R)[1][0]
    assert d_last == want[1][0] and li.land_images_numpy(rects[1:2], segs[:1], R)[1][0] == want[1][1]
    for n in (1, 4, 5):
        t = {}
        got = gpu(rects[:n], segs, R, 1000.0, times=t)
        assert t["nbands"] == 1 and t["entries"] == E
        same(got, (want[0][:n], want[1][:n]), (E, n))


def test_an_edge_exactly_three_indents_away_in_and_out_of_the_searched_bands(lib):
    """cap2 = (2 r)^2 and a reach of 3 r: an edge 3 r of y away is searched or not, depending on the band height, and gives the cap either way."""
    rect = np.asarray([[0.0, 0, 10, 10]]) + [OX, OY, OX, OY]
    up = np.nextafter(OY + 25.0, np.inf) - OY
    for gap_edges, want_d2 in (([25.0], CAP2), ([up], CAP2), ([26.0], CAP2), ([-15.0], CAP2), ([-16.0], CAP2), ([20.0], CAP2), ([19.875], 9.875 ** 2),
                               ([-9.875], 9.875 ** 2), ([14.0], 16.0), ([25.0, -9.875], 9.875 ** 2), ([up, 19.875, -40.0], 9.875 ** 2)):
        segs = np.asarray([[-5.0, y, 15.0, y] for y in gap_edges] + [[-5.0, -60.0, 15.0, -60.0], [-5.0, 70.0, 15.0, 70.0]]) + [OX, OY, OX, OY]
        want = li.land_images_numpy(rect, segs, R)
        assert want[1].tolist() == [want_d2] and want[0].tolist() == [1 if want_d2 < 25 else 0], (gap_edges, want)
        for bh in (None, 0.5, 1.0, 5.0, 7.0, 15.0, 1000.0):
            same(gpu(rect, segs, R, bh), want, (gap_edges, bh))


def test_rectangles_outside_all_bands_a_reach_over_every_band_and_rectangles_that_are_no_numbers(lib):
    rects, segs = star_case()
    top, bottom = float(max(segs[:, 1].max(), segs[:, 3].max())), float(min(segs[:, 1].min(), segs[:, 3].min()))
    nan, inf = float("nan"), float("inf")
    odd = np.asarray([[OX, top + 100, OX + 10, top + 110], [OX, bottom - 110, OX + 10, bottom - 100],        # above and below all bands
                      [OX, top + 4, OX + 10, top + 14], [OX, bottom - 14, OX + 10, bottom - 4],                # outside them, within the reach
                      [OX, top + 15, OX + 10, top + 25], [OX, bottom - 25, OX + 10, bottom - 15],              # exactly the reach away
                      [nan, OY, OX + 10, OY + 10], [OX, nan, OX + 10, OY + 10], [OX, OY, nan, OY + 10], [OX, OY, OX + 10, nan], [nan] * 4,
                      [OX, OY, OX + 10, inf], [OX, -inf, OX + 10, OY], [OX, inf, OX + 10, inf], [-inf, -inf, inf, inf],
                      [OX, bottom - 1000, OX + 1, top + 1000]])                                                # through every band
    both = np.concatenate([odd, rects[:200]])
    for r, bh in ((R, None), (R, 0.5), (R, 7.0), (1.0e4, None), (1.0e4, 7.0), (0.01, None)):   # 3 x 1e4 m reaches every band from anywhere
        want = li.land_images_numpy(both, segs, r)
        same(gpu(both, segs, r, bh), want, (r, bh))
        assert want[0][6:11].tolist() == [0] * 5 and want[1][6:11].tolist() == [(2 * r) * (2 * r)] * 5      # a coordinate that is not a number
    far = li.land_images_numpy(both, segs, R)
    assert far[0][:2].tolist() == [0, 0] and far[1][:2].tolist() == [CAP2, CAP2] and far[0][15] == 1 and far[1][15] == 0.0


def test_no_rectangles_and_no_land(lib):
    rects, segs = star_case()
    f, d = gpu(np.zeros((0, 4)), segs)
    assert f.shape == (0,) and d.shape == (0,)
    f, d = gpu(rects[:101], np.zeros((0, 4)))
    assert f.tolist() == [0] * 101 and d.tolist() == [CAP2] * 101
    f, d = gpu(rects[:3], np.zeros((0, 4)), 1.5)
    assert f.tolist() == [0] * 3 and d.tolist() == [9.0] * 3
    assert gpu(np.zeros((0, 4)), np.zeros((0, 4)))[0].shape == (0,)
    assert li.land_images_gpu(np.zeros((0, 4)), segs)[1].shape == (0,)


def test_the_same_bytes_twice(lib):
    from aquaculture_amd.engine import land_images
    rects, segs = star_case()
    b, s = torch.from_numpy(rects).cuda(), torch.from_numpy(segs).cuda()
    (f1, d1), (f2, d2) = land_images(b, s, R), land_images(b, s, R)
    assert torch.equal(f1, f2) and torch.equal(d1.view(torch.int64), d2.view(torch.int64))


def test_bad_arguments_are_refused_and_both_outputs_stay_untouched(lib):
    from aquaculture_amd import engine
    rects, segs = star_case()
    rects = rects[:9]
    N, E = rects.shape[0], segs.shape[0]
    b, s = torch.from_numpy(rects).cuda(), torch.from_numpy(segs).cuda()
    entry_seg, band_start, nbands, Y0, h = engine.land_band_table(s)
    entries = entry_seg.shape[0]
    need = int(lib.aq_land_images_scratch_bytes(entries))
    assert need == 32 * entries
    scratch = torch.full((need + 32,), 0x5A, dtype=torch.uint8, device="cuda")
    flags = torch.full((N + 8,), 0x77, dtype=torch.uint8, device="cuda")
    dist2 = torch.full((N + 8,), -7.0, dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def call(seg_p=s.data_ptr(), E_=E, entry_p=entry_seg.data_ptr(), entries_=entries, start_p=band_start.data_ptr(), nbands_=nbands, Y0_=Y0, h_=h,
             rects_p=b.data_ptr(), N_=N, indent_=R, scratch_p=scratch.data_ptr(), scratch_bytes=need, flags_p=flags.data_ptr(), dist2_p=dist2.data_ptr()):
        return lib.aq_land_images_f64(seg_p, E_, entry_p, entries_, start_p, nbands_, Y0_, h_, rects_p, N_, indent_, scratch_p, scratch_bytes, flags_p,
                                      dist2_p, stream)

    untouched = lambda: bool((flags == 0x77).all()) and bool((dist2 == -7.0).all()) and bool((scratch == 0x5A).all())
    for kw, msg in (({"indent_": 0.0}, "indent"), ({"indent_": -5.0}, "indent"), ({"indent_": float("nan")}, "indent"), ({"indent_": float("inf")}, "indent"),
                    ({"h_": 0.0}, "band height"), ({"h_": float("nan")}, "band height"), ({"h_": float("inf")}, "band height"),
                    ({"Y0_": float("nan")}, "Y0"), ({"Y0_": float("-inf")}, "Y0"), ({"nbands_": 0}, "nbands"),
                    ({"seg_p": None}, "null pointer"), ({"entry_p": None}, "null pointer"), ({"start_p": None}, "null pointer"),
                    ({"rects_p": None}, "null pointer"), ({"scratch_p": None}, "null pointer"), ({"flags_p": None}, "null pointer"),
                    ({"dist2_p": None}, "null pointer"), ({"dist2_p": None, "E_": 0}, "null pointer"), ({"flags_p": None, "entries_": 0}, "null pointer"),
                    ({"seg_p": s.data_ptr() + 8}, "unaligned"), ({"rects_p": b.data_ptr() + 16}, "unaligned"), ({"scratch_p": scratch.data_ptr() + 8}, "unaligned"),
                    ({"entry_p": entry_seg.data_ptr() + 2}, "unaligned"), ({"dist2_p": dist2.data_ptr() + 4}, "unaligned"),
                    ({"E_": 1 << 31}, "2\\^31"), ({"N_": 1 << 31}, "2\\^31"), ({"entries_": 1 << 31}, "2\\^31"), ({"E_": -1}, "2\\^31"),
                    ({"scratch_bytes": need - 1}, "scratch")):
        assert call(**kw) == -1, kw
        assert re.search(msg, lib.aq_last_error().decode()), (kw, lib.aq_last_error())
        torch.cuda.synchronize()
        assert untouched(), kw
    # N = 0 does nothing, whatever the pointers
    assert lib.aq_land_images_f64(None, E, None, entries, None, nbands, Y0, h, None, 0, R, None, 0, None, None, stream) == 0
    torch.cuda.synchronize()
    assert untouched()
    with pytest.raises(ValueError, match="indent"):
        engine.land_images(b, s, 0.0)
    with pytest.raises(ValueError, match="band height"):
        engine.land_images(b, s, R, 0.0)
    with pytest.raises(ValueError, match=r"\d{10,} band entries"):
        engine.land_images(b, s, R, 1e-9)
    torch.cuda.synchronize()
    assert untouched()
    want = li.land_images_numpy(rects, segs, R)
    assert call() == 0                                      # and the same arguments, all valid, run
    torch.cuda.synchronize()
    same((flags[:N].cpu().numpy(), dist2[:N].cpu().numpy()), want, "the valid call")
    assert bool((flags[N:] == 0x77).all()) and bool((dist2[N:] == -7.0).all()) and bool((scratch[need:] == 0x5A).all())
    # E = 0 needs no table: byte 0 and the cap, in [N] only
    assert lib.aq_land_images_f64(None, 0, None, 0, None, 1, 0.0, 1.0, None, N, R, None, 0, flags.data_ptr(), dist2.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    assert bool((flags[:N] == 0).all()) and bool((dist2[:N] == CAP2).all()) and bool((flags[N:] == 0x77).all()) and bool((dist2[N:] == -7.0).all())


# ---- python -m aquaculture_amd.land --images ----

def test_command_line_gpu_and_cpu_write_the_same_files(lib, tmp_path):
    labels, csv_path, land_path = label_run(tmp_path)
    (tmp_path / "images.txt").write_text("".join(n + "\n" for n in all_images(labels)))
    outs = []
    for extra in ([], ["--cpu"]):
        out = tmp_path / ("out" + "".join(extra))
        r = subprocess.run(["timeout", "-k", "10", "150", sys.executable, "-m", "aquaculture_amd.land", "--labels", labels, "--geocode-bboxes", csv_path,
                            "--land", land_path, "--images", str(tmp_path / "images.txt"), "--out", str(out), *extra], cwd=ROOT, capture_output=True,
                           text=True, timeout=180)
        assert r.returncode == 0, r.stderr[-3000:]
        assert re.search(r"6 of 12 images wholly on land, 5 m or more from the coast \(7 land edges", r.stdout), r.stdout
        outs.append((open(out / li.CSV_FILE).read(), open(out / li.JSON_FILE).read()))
    assert outs[0][0] == outs[1][0] and outs[0][0].count("True,True") == 6
    assert re.sub(r'"device": "[^"]*"', "", outs[0][1]) == re.sub(r'"device": "[^"]*"', "", outs[1][1]) and '"device": "cpu"' in outs[1][1]


# ---- detect.py --land-images ----

def test_detect_py_marks_the_images_of_its_source(lib, tmp_path):
    """An engine sweep over four synthetic 640-px tiles with the synthetic checkpoint, geocoded and land-filtered in the same run: the two
    files are what the host restatement makes of the source's listing; the western tile of the four lies on land."""
    import json
    from PIL import Image
    from test_gpu_facilities import synthetic_run
    from test_land_filter import lonlat_ring
    from aquaculture_amd import checkpoint, geocode, kfold, land, tiles
    (tmp_path / "jpegs").mkdir()
    names = [f"ORTHOIMAGERY.ORTHOPHOTOS{2015 - k % 2}_3_{1024 * k}_0" for k in range(4)]
    for k, i in enumerate((0, 3, 19, 20)):
        Image.fromarray(tiles.synthetic_tile(i, 640)).save(tmp_path / "jpegs" / (names[k] + ".jpeg"), quality=95)
    checkpoint.write_synthetic_checkpoint(str(tmp_path / "synth.pt"), "yolov5m", 5)
    _, csv_path = synthetic_run(tmp_path)
    x0, y0 = (float(v) for v in geocode.lonlat_to_mercator(np.float64(3.5), np.float64(43.3)))
    west = [(x0 - 50, y0 - 50), (x0 + 400, y0 - 50), (x0 + 500, y0 + 1900), (x0 - 50, y0 + 1900)]      # the scene's western quarter is land
    land_path = tmp_path / "land.geojson"
    land_path.write_text(json.dumps({"type": "Polygon", "coordinates": [lonlat_ring(west)]}))
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "yolov5", "detect.py"), "--weights", str(tmp_path / "synth.pt"),
                        "--source", str(tmp_path / "jpegs"), "--save-txt", "--save-conf", "--nosave", "--project", str(tmp_path / "runs"), "--name", "land",
                        "--batch-size", "4", "--geocode-bboxes", csv_path, "--land-filter", str(land_path), "--land-images"],
                       capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    run = tmp_path / "runs" / "land"
    assert "1 of 4 images wholly on land, 5 m or more from the coast (4 land edges; 0 within 2 % of the indent)" in r.stdout + r.stderr
    assert "land_images" not in json.load(open(run / "run_params.json"))
    rect_of = kfold.tile_rects(csv_path)
    want = li.land_images_numpy(np.asarray([rect_of(n) for n in sorted(names)]), land.load_land_geojson(str(land_path)), R)
    li.write_csv(str(tmp_path / "want.csv"), sorted(names), *want)
    assert open(run / li.CSV_FILE).read() == open(tmp_path / "want.csv").read()
    back = li.read_csv(str(run / li.CSV_FILE))
    assert back["on_land"] == [n.endswith("_3_0_0") for n in sorted(names)]
    s = json.load(open(run / li.JSON_FILE))
    assert s["on_land"] == 1 and s["images"] == 4 and s["device"] != "cpu" and s["by_byte"] == {str(b): int((want[0] == b).sum()) for b in range(4)}
