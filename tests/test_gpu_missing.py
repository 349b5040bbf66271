"""--tonnage-missing on the GPU: csrc/coverage.hip gives missing.first_numpy's bytes on the hand cases and the random cases of
tests/test_missing.py, at the run lengths, ring lengths and query counts around a wavefront, on an enlarged case twice, and on slices of
larger arrays; the launcher refuses by its arguments alone; nothing depends on bytes the kernel does not own; both command lines write the
--cpu route's files."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_dedup import synthetic_sweep
from test_missing import EXACT, FACTORS, blob_ring, hand_cases, literal_case, make_reg, px_box, run_cli, sites_csv, stem, sweep, tiles_case

from aquaculture_amd import engine, missing as ms, tonnage as tn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same(reg, boxes, qpass, nbands=(None,)):
    """first_gpu against first_numpy through the same band tables, byte for byte."""
    for nb in nbands:
        t = ms.band_tables(reg, nb)
        got, want = ms.first_gpu(reg, t, boxes, qpass), ms.first_numpy(reg, t, boxes, qpass)
        assert got.dtype == want.dtype == np.int32 and got.tobytes() == want.tobytes(), (nb, np.nonzero(got != want)[0][:10].tolist())
    return got


def test_hand_cases_are_the_restatements_bytes(lib):
    for name, reg, boxes, qpass, want in hand_cases():
        assert same(reg, boxes, qpass, (None, 1, 3)).tolist() == want, name
    empty = ms.regions([], {}, EXACT)
    assert same(empty, [px_box(0, 0, 1, 1)] * 5, [0, -1, 1, 0, 0]).tolist() == [-1] * 5
    assert same(hand_cases()[0][1], np.zeros((0, 4)), np.zeros(0, np.int32)).shape == (0,)


def test_random_cases_of_the_cpu_suite(lib):
    reg, boxes, qpass, closed, _ = literal_case()
    assert ((same(reg, boxes, qpass, (None, 1)) >= 0) == closed).all()
    reg, boxes, qpass = tiles_case()
    got = same(reg, boxes, qpass, (1, 7, None))
    assert (got == ms.first_bruteforce(reg, boxes, qpass)).all()
    for n in (1, 3, 4, 5):                                  # a block holds four queries
        assert (same(reg, boxes[40:40 + n], qpass[40:40 + n]) == got[40:40 + n]).all()


def test_run_lengths_around_a_wavefront(lib):
    """Passes of 1, 63, 64, 65 and 130 complete tiles side by side in one band, so a query's run is the whole pass; only one image meets
    each box, at every position of the run, last lanes included.  A run of no entry: a band no image is in."""
    years, counts = (2002, 2007, 2011, 2014, 2017), (1, 63, 64, 65, 130)
    wanted = {k: (6144.0 * k, 0.0, 6144.0 * (k + 1), 6144.0) for k in range(22)}
    images = [(stem(y, ind=k // 6, xo=1024 * (k % 6)), None) for y, n in zip(years, counts) for k in range(n)]
    reg = make_reg(images, wanted)
    assert np.diff(reg["pass_start"]).tolist() == list(counts)
    boxes, qpass = [], []
    for p, n in enumerate(counts):
        for i in range(int(reg["pass_start"][p]), int(reg["pass_start"][p + 1])):
            w, s, e, _ = reg["rect"][i].tolist()
            boxes += [(w + 10.0, s + 10.0, w + 20.0, s + 20.0), (w + 10.0, s - 20.0, w + 20.0, s - 10.0)]
            qpass += [p, p]
        boxes.append((-10.0, 5130.0, 1e9, 5140.0))          # meets every image of the pass: the first one
        qpass.append(p)
    t = ms.band_tables(reg, 1)
    assert np.diff(t["band_start"]).tolist() == list(counts)
    got = same(reg, boxes, qpass, (1,))
    assert (got >= 0).sum() == sum(counts) + len(counts) and sorted(set(got[got >= 0].tolist())) == list(range(sum(counts)))
    tall = make_reg([(stem(2014), None), (stem(2014, yo=5120), None)])          # two tiles, three empty bands between them
    t = ms.band_tables(tall, 6)
    assert np.diff(t["band_start"]).tolist() == [1, 1, 0, 0, 0, 1]               # (the lower tile's north edge is the first line of band 1)
    assert same(tall, [px_box(10, 2000, 20, 2010), px_box(10, 1000, 20, 1030), px_box(10, 100, 20, 6000)], [0, 0, 0], (6,)).tolist() == [-1, 0, 0]


def staircase(steps, extra, size=8):
    """A closed walk of 2 steps + 2 + extra segments: stairs down to the right, back along the bottom and up the left side, which `extra`
    more vertices cut into collinear pieces."""
    ring = [(0, 0)]
    for j in range(steps):
        ring += [((j + 1) * size, j * size), ((j + 1) * size, (j + 1) * size)]
    ring.append((0, steps * size))
    ring += [(0, steps * size - 1 - k) for k in range(extra)]
    return ring + [(0, 0)]


def test_ring_lengths_around_a_wavefront(lib):
    shapes = {4: [(0, 0), (8, 0), (8, 8), (0, 8), (0, 0)], 63: staircase(30, 1), 64: staircase(31, 0), 65: staircase(31, 1), 129: staircase(63, 1),
              128: staircase(63, 0)}
    years = (2002, 2007, 2011, 2014, 2017, 2020)
    reg = make_reg([(stem(y), shapes[n]) for y, n in zip(years, shapes)])
    assert (np.diff(reg["ring_start"]) - 1).tolist() == list(shapes)
    boxes, qpass = [], []
    for p, (n, ring) in enumerate(shapes.items()):
        steps = max(v[1] for v in ring) // 8
        for j in range(steps + 1):
            x, y = 8.0 * j, 8.0 * j
            boxes += [px_box(x + 8.5, y - 4, x + 12, y - 0.5),                 # above the stairs, beside step j: outside
                      px_box(x + 8, y - 4, x + 12, y),                         # touching step j's corner
                      px_box(x + 1, y + 1, x + 3, y + 3) if j < steps else px_box(0, y, 0, y),   # inside under step j: the parity decides
                      px_box(-5, y + 2, -0.5, y + 3), px_box(-5, y + 2, 0, y + 3)]               # left of the left side: beside it, touching it
            qpass += [p] * 5
        boxes += [px_box(1, steps * 8 + 0.5, 5, steps * 8 + 3), px_box(1, steps * 8, 5, steps * 8 + 3)]   # under the bottom side
        qpass += [p, p]
    got = same(reg, boxes, qpass, (None, 1))
    assert (got == ms.first_bruteforce(reg, boxes, qpass)).all() and 0.3 < (got >= 0).mean() < 0.8


@functools.lru_cache(None)
def large_case():
    """6 passes of 500 tiles (14 download boxes near y = 5.3e6 m, some over each other), a fifth of them with one of 16 blob rings, one with
    the ring of a 1024 x 1024 noise pattern; 20,000 boxes of a few metres over the area and around it."""
    rng = np.random.default_rng(2024)
    base = (655956.8325696054, 5325167.07623245)
    wanted = {k: (base[0] + 1200.0 * (k % 5) + 400.0 * (k // 5), base[1] - 1200.0 * (k // 5) - 300.0 * (k % 2),
                  base[0] + 1200.0 * (k % 5) + 400.0 * (k // 5) + 1200.0, base[1] - 1200.0 * (k // 5) - 300.0 * (k % 2) + 1200.0) for k in range(14)}
    rings = [blob_ring(rng, int(c)) for c in (4, 8, 8, 8, 16, 16, 16, 16, 32, 32, 32, 32, 64, 64, 64, 128)]
    big = blob_ring(rng, 512)
    assert len(big) >= 5000
    images = []
    for year in (2002, 2007, 2011, 2014, 2017, 2020):
        tiles = [(k, xo, yo) for k in range(14) for xo in range(0, 6144, 1024) for yo in range(0, 6144, 1024)]
        for j in rng.permutation(len(tiles))[:500].tolist():
            images.append((stem(year, *tiles[j]), rings[int(rng.integers(0, 16))] if rng.random() < 0.2 else None))
    images[1234] = (images[1234][0], big)
    reg = make_reg(images, wanted)
    lo, hi = reg["rect"][:, :2].min(0) - 200.0, reg["rect"][:, 2:].max(0) + 200.0
    corner = lo + rng.random((20000, 2)) * (hi - lo)
    k = int(np.nonzero(reg["kind"] & (np.diff(reg["ring_start"]) >= 5000))[0][0])
    corner[:2000] = reg["rect"][k, :2] + rng.random((2000, 2)) * (reg["rect"][k, 2:] - reg["rect"][k, :2])      # on the tile of the large ring
    boxes = np.concatenate([corner, corner + rng.random((20000, 2)) * np.asarray([6.0, 6.0]) * (rng.random((20000, 1)) < 0.9)], 1)
    qpass = rng.integers(0, 6, 20000).astype(np.int32)
    qpass[:2000] = reg["pass_id"][k]
    qpass[rng.random(20000) < 0.01] = -1
    t = ms.band_tables(reg)
    return reg, t, boxes, qpass, ms.first_numpy(reg, t, boxes, qpass)


def test_large_case_twice(lib):
    reg, t, boxes, qpass, want = large_case()
    assert reg["rect"].shape[0] == 3000 and len(reg["passes"]) == 6 and 500 < reg["kind"].sum() < 700 and np.diff(reg["ring_start"]).max() >= 5000
    assert t["nbands"] == 62 and 0.2 < (want >= 0).mean() < 0.9 and len(set(want.tolist())) > 1000
    a, b = ms.first_gpu(reg, t, boxes, qpass), ms.first_gpu(reg, t, boxes, qpass)
    assert a.tobytes() == b.tobytes() == want.tobytes()


def test_slices_of_larger_arrays(lib):
    """The queries from row 5 on, and the images of pass 3 alone with ring starts that do not begin at 0, as views of the whole arrays."""
    reg, t, boxes, qpass, want = large_case()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d = {k: dev(reg[k]) for k in ("rect", "ring_start", "xy")}
    d.update({k: dev(t[k]) for k in ("entry_img", "band_start", "band")})
    bq, pq = dev(boxes), dev(qpass)
    got = engine.coverage_first(d["rect"], d["ring_start"], d["xy"], d["entry_img"], d["band_start"], d["band"], t["nbands"], bq[5:1005], pq[5:1005],
                                reg["ring_start"], t["band_start"], t["band"])
    assert got.cpu().numpy().tobytes() == want[5:1005].tobytes()
    i0, i1 = int(reg["pass_start"][3]), int(reg["pass_start"][4])
    assert reg["ring_start"][i0] > 0
    sub = {"passes": [reg["passes"][3]], "pass_id": np.zeros(i1 - i0, np.int32), "pass_start": np.asarray([0, i1 - i0], np.int32), "rect": reg["rect"][i0:i1],
           "kind": reg["kind"][i0:i1], "ring_start": reg["ring_start"][i0:i1 + 1], "xy": reg["xy"], "names": reg["names"][i0:i1]}
    ts = ms.band_tables(sub)
    q = np.nonzero(qpass == 3)[0]
    want_sub = ms.first_numpy(sub, ts, boxes[q], np.zeros(q.shape[0], np.int32))
    assert (np.where(want_sub >= 0, want_sub + i0, -1) == want[q]).all()
    got = engine.coverage_first(d["rect"][i0:i1], d["ring_start"][i0:i1 + 1], d["xy"], dev(ts["entry_img"]), dev(ts["band_start"]), dev(ts["band"]), ts["nbands"],
                                dev(boxes[q]), dev(np.zeros(q.shape[0], np.int32)), sub["ring_start"], ts["band_start"], ts["band"])
    assert got.cpu().numpy().tobytes() == want_sub.tobytes()


def test_launcher_refuses_by_its_arguments(lib):
    f = lib.aq_coverage_first_i32
    i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)
    f64 = lambda v: np.ascontiguousarray(v, dtype=np.float64)
    z = lambda shape, dt=torch.int32: torch.zeros(shape, dtype=dt, device="cuda")
    box, qp, first, scratch = z((4, 4), torch.float64), z(4), z(4), z(1024, torch.uint8)
    rect, rsd, xy, entry, bsd, band = z((2, 4), torch.float64), z(3), z((5, 2), torch.float64), z(2), z(3), z((1, 2), torch.float64)

    def call(ring_start=(0, 0, 5), band_start=(0, 1, 2), band_host=((0.0, 1.0),), I=2, V=5, entries=2, P=1, nbands=2, Q=4, scratch_bytes=1024, null=False):
        rs, bs, bh = i32(ring_start), i32(band_start), f64(band_host)
        p = (lambda t_: None) if null else (lambda t_: t_.data_ptr())
        rc = f(p(rect), p(rsd), rs.ctypes.data, I, p(xy), V, p(entry), entries, p(bsd), bs.ctypes.data, p(band), bh.ctypes.data, P, nbands, p(box), p(qp), Q,
               p(scratch), scratch_bytes, p(first), None)
        return rc, lib.aq_last_error()

    for (rc, msg), text in ((call(I=-1), b"-1 images"), (call(entries=-1), b"-1 band entries"), (call(Q=-1), b"-1 queries"), (call(P=-1), b"-1 passes"),
                            (call(V=-1), b"-1 ring vertices"), (call(V=1 << 31), b"2147483648 ring vertices"), (call(I=1 << 31), b"2147483648 images"),
                            (call(Q=1 << 31), b"2147483648 queries"), (call(entries=1 << 31), b"2147483648 band entries"),
                            (call(nbands=0), b"0 bands"), (call(nbands=-3), b"-3 bands"), (call(P=1 << 20, nbands=1 << 11), b"2048 bands for each of 1048576 passes"),
                            (call(ring_start=(0, 5, 3)), b"ring starts are not sorted at image 1"), (call(ring_start=(0, 0, 6)), b"ring starts 0 .. 6 leave the 5 vertices"),
                            (call(ring_start=(-1, 0, 5)), b"ring starts -1 .. 5"), (call(band_start=(0, 2, 1)), b"band starts are not sorted at pass 0, band 1"),
                            (call(band_start=(0, 1, 3)), b"band starts 0 .. 3 leave the 2 entries"), (call(band_start=(-1, 1, 2)), b"band starts -1 .. 2"),
                            (call(band_host=((0.0, 0.0),)), b"band height h = 0"), (call(band_host=((0.0, float("nan")),)), b"pass 0 has Y0 = 0"),
                            (call(band_host=((float("inf"), 1.0),)), b"pass 0 has Y0 = inf"), (call(scratch_bytes=63), b"63 bytes of scratch, 64 needed"),
                            (call(null=True), b"null pointer")):
        assert rc != 0 and msg.startswith(b"coverage:") and text in msg, (text, msg)
    first.fill_(7)
    assert call(Q=0)[0] == 0 and call(Q=0, null=True)[0] == 0 and first.tolist() == [7] * 4          # nothing to do, nothing written
    assert call()[0] == 0 and first.tolist() == [-1] * 4                                             # (all-zero tables: nothing meets)
    # the binding checks what it is given, and the library's refusal comes back as an error
    args = lambda **kw: {**dict(rect=rect, ring_start=rsd, xy=xy, entry_img=entry, band_start=bsd, band=band, nbands=2, box=box, qpass=qp,
                                ring_start_host=[0, 0, 5], band_start_host=[0, 1, 2], band_host=[[0.0, 1.0]]), **kw}
    with pytest.raises(ValueError, match="contiguous CUDA"):
        engine.coverage_first(**args(qpass=z(4, torch.int64)))
    with pytest.raises(ValueError, match="contiguous CUDA"):
        engine.coverage_first(**args(box=z((4, 4), torch.float64).cpu()))
    with pytest.raises(ValueError, match="contiguous CUDA"):
        engine.coverage_first(**args(band_start=z(4)))
    for kw in (dict(ring_start_host=[0, 5]), dict(band_start_host=[0, 1, 2, 2]), dict(band_host=[[0.0, 1.0], [0.0, 1.0]])):
        with pytest.raises(ValueError, match="host copies"):
            engine.coverage_first(**args(**kw))
    with pytest.raises(RuntimeError, match="coverage: ring starts are not sorted"):
        engine.coverage_first(**args(ring_start_host=[0, 5, 3]))


def test_result_does_not_depend_on_bytes_it_does_not_own(lib, monkeypatch):
    from poison import poisoned
    reg, boxes, qpass = tiles_case()
    t = ms.band_tables(reg, 7)
    want = ms.first_numpy(reg, t, boxes, qpass)
    for byte in (0xFF, 0x00, 0x5A):
        with poisoned(monkeypatch, byte) as p:
            got = ms.first_gpu(reg, t, boxes, qpass)
            torch.cuda.synchronize()
            p.check_guards()                                # first and the scratch: nothing written past either
            assert p.intercepted >= 2 and not p.passed_through
        assert got.tobytes() == want.tobytes(), hex(byte)


# ---- the command lines ----

SAME = (tn.ESTIMATES_FILE, tn.FACILITIES_FILE, ms.CAGES_FILE, ms.FACILITIES_FILE, ms.NEAR_FILE)


def test_module_command_line_writes_the_cpu_runs_bytes(lib, tmp_path):
    s = sweep(tmp_path)
    (tmp_path / "factors.csv").write_text(FACTORS)
    sites = sites_csv(tmp_path, s["table"])
    more = ["--dedup-years", s["key"], s["geom"], "--tonnage-missing", "--tonnage-near-sites", sites]
    want = run_cli(s, tmp_path, "cpu", *more)
    r = subprocess.run([sys.executable, "-m", "aquaculture_amd.tonnage", "--labels", s["labels"], "--geocode-bboxes", s["bboxes"], "--tonnage-factors",
                        str(tmp_path / "factors.csv"), "--tonnage-K", "64", "--tonnage-seed", "7", "--out", str(tmp_path / "gpu"), *more],
                       cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    for f in SAME:
        assert open(tmp_path / "gpu" / f, "rb").read() == open(want / f, "rb").read(), f
    a, b = json.load(open(tmp_path / "gpu" / tn.JSON_FILE)), json.load(open(want / tn.JSON_FILE))
    assert a["missing"] == b["missing"] and a["near_sites"] == b["near_sites"] and not a["cpu"] and b["cpu"]
    assert len(open(want / tn.ESTIMATES_FILE).read().splitlines()) == 1 + 3 + 5 and "with missing imagery" in r.stdout


def test_detect_py_fills_in_the_missing_imagery_of_its_own_sweep(lib, tmp_path):
    """The tiny sweep of tests/test_gpu_dedup.py: four tiles in 2014 and 2015, one once more in 2013 with its right part white, one in 2017.
    Each of the two passes takes from the other; the files equal what the --cpu route makes of the run's labels, key and outlines."""
    from PIL import Image
    from aquaculture_amd import checkpoint, dedup as dd, geocode, tiles
    (tmp_path / "jpegs").mkdir()
    save = lambda arr, year, k: Image.fromarray(arr).save(tmp_path / "jpegs" / f"ORTHOIMAGERY.ORTHOPHOTOS{year}_3_{1024 * k}_0.jpeg", quality=95)
    for k, i in enumerate((0, 3, 19, 20)):
        for year in (2014, 2015):
            save(tiles.synthetic_tile(i, 640), year, k)
    white = tiles.synthetic_tile(0, 640).copy()
    white[:, 400:] = 255
    save(white, 2013, 0)
    save(tiles.synthetic_tile(3, 640), 2017, 0)
    checkpoint.write_synthetic_checkpoint(str(tmp_path / "synth.pt"), "yolov5m", 5)
    _, csv_path = synthetic_sweep(tmp_path)
    (tmp_path / "factors.csv").write_text("pass,s_mean,s_sd,h_mean,h_sd\n2013-2015,12,3,0.8,0.1\n2016-2018,12,3,0.8,0.1\n")
    (tmp_path / "sites.csv").write_text("lat,lon\n43.31,3.5\n")
    conf = ["--facilities-conf", "0.25", "--facilities-eps", "25", "--facilities-min-cages", "4"]
    cmap = "2013-2015=2016-2018,2016-2018=2013-2015"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "yolov5", "detect.py"), "--weights", str(tmp_path / "synth.pt"), "--source",
                        str(tmp_path / "jpegs"), "--save-txt", "--save-conf", "--nosave", "--project", str(tmp_path / "runs"), "--name", "dd",
                        "--batch-size", "4", "--geocode-bboxes", csv_path, *conf, "--tonnage", "--tonnage-factors", str(tmp_path / "factors.csv"),
                        "--tonnage-K", "200", "--dedup-years", "--dedup-selection", "max", "--dedup-seed", "3", "--tonnage-missing", cmap,
                        "--tonnage-near-sites", str(tmp_path / "sites.csv")], capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    run = tmp_path / "runs" / "dd"
    labels, key, geom = str(run / "labels"), str(run / "image_boxes_blank_key.csv"), str(run / "image_boxes_partly_blank.geojson")
    table = geocode.geocode_label_dir(labels, csv_path)
    res = dd.dedup_from_table(table, key, geom, None, "max", 3, 0.25, None, 640, 640, cpu=True)
    tn.tonnage_from_table(table, str(tmp_path / "want"), str(tmp_path / "factors.csv"), K=200, conf_thresh=0.25, eps=25.0, min_cages=4, widths=640, heights=640,
                          cpu=True, dedup=res, missing=ms.settings(cmap, key, geom, csv_path), near_sites=str(tmp_path / "sites.csv"))
    for f in SAME:
        assert open(run / f, "rb").read() == open(tmp_path / "want" / f, "rb").read(), f
    rows = open(run / tn.ESTIMATES_FILE).read().splitlines()
    assert [x.split(",")[0] for x in rows[1:]] == ["Model"] * 2 + [ms.SOURCE] * 2 and len(open(run / ms.CAGES_FILE).read().splitlines()) > 1
    assert "missing" not in open(run / "run_params.json").read()
