"""--dedup-years on the GPU: csrc/dedup.hip gives the bytes of dedup.fill_numpy / sets_numpy / select_numpy -- bitmaps, set words, selection
bits, chosen orders and all n! area sums -- on the hand cases of tests/test_dedup.py and on an enlarged random case; the launchers refuse
by their arguments alone; both command lines write the --cpu route's files."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_dedup import ALL, WINDOW_PIXELS, fill_problem, hand_problems, random_case, random_problem, synthetic_sweep, window_problem

from aquaculture_amd import dedup as dd, engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_run(p, budget=dd.BUDGET_BYTES):
    """selections_gpu against selections_numpy: every array of the result and, per chunk, the bitmap and the set words, byte for byte."""
    dg, dn = [], []
    got, want = dd.selections_gpu(p, budget, dg), dd.selections_numpy(p, budget, dn)
    for k in ("bits", "chosen", "sums"):
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k
    assert len(dg) == len(dn)
    for a, b in zip(dg, dn):
        assert a["groups"] == b["groups"]
        for k in ("bitmap", "words"):
            assert a[k].dtype == b[k].dtype == np.uint32 and a[k].tobytes() == b[k].tobytes(), (k, a["groups"])
    return got


def test_hand_cases_are_the_restatements_bytes(lib):
    p, _ = fill_problem()
    same_run(p)
    for w, h, px, py in WINDOW_PIXELS:
        p, want = window_problem(w, h, px, py)
        assert ((same_run(p)["bits"] == ALL) == want).all()
    for name, (p, bits, (qmin, qmax), sums) in hand_problems().items():
        got = same_run(p)
        assert got["bits"].tolist() == bits and got["chosen"][0, :2].tolist() == [qmin, qmax] and got["sums"][0, :len(sums)].tolist() == sums, name


def test_random_case_of_the_cpu_suite(lib):
    p, want, _ = random_case()
    got = same_run(p)
    assert all((got[k] == want[k]).all() for k in want)
    same_run(p, 40000)                                      # in chunks of a few groups


@functools.lru_cache(maxsize=None)
def large_case():
    """2,000 groups and 20,000 cages on 96 x 72 frames; group 7 has five blob images of 1024 x 1024 (the real row pitch of 33 words) and
    400 of the cages."""
    p = random_problem(77, 2000, 20000, big=(7, 1024))
    t = dd.tables(p)
    bitmap = dd.fill_numpy(t["ring_xy"], t["ring_start"], t["ring_frame"], t["bitmap_words"])
    words = dd.sets_numpy(t["group"], t["cage"], bitmap)
    return p, t, bitmap, words, dd.select_numpy(t["group"], t["cage_start"], t["cage"], words, t["area"], t["random_order"])


def launches(t, rings=slice(None), cages=slice(None), groups=slice(None)):
    """The three launchers on the tables t -- or on a slice of the rings (fill), of the cages (sets) and of the groups (select), the other
    arrays whole, so that ring_start, the cage pointer and cage_start do not start at 0 -> host arrays."""
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d = {k: dev(t[k]) for k in ("ring_xy", "ring_start", "ring_frame", "group", "cage", "cage_start", "area", "random_order")}
    R, G = t["ring_frame"].shape[0], t["group"].shape[0]
    r0, r1, _ = rings.indices(R)
    g0, g1, _ = groups.indices(G)
    bitmap = torch.zeros(int(t["bitmap_words"]), dtype=torch.int32, device="cuda")
    engine.dedup_fill(d["ring_xy"], d["ring_start"][r0:r1 + 1], d["ring_frame"][r0:r1], bitmap, t["ring_start"][r0:r1 + 1], t["ring_frame"][r0:r1])
    words = engine.dedup_sets(d["group"], d["cage"][cages], bitmap, t["group"])
    full = torch.zeros(t["cage"].shape[0], dtype=torch.int32, device="cuda")
    full[cages] = words
    sel, chosen, sums = engine.dedup_select(d["group"][g0:g1], d["cage_start"][g0:g1 + 1], d["cage"], full, d["area"], d["random_order"][g0:g1],
                                            t["group"][g0:g1], t["cage_start"][g0:g1 + 1])
    return tuple(x.cpu().numpy() for x in (bitmap, words, sel, chosen, sums))


def test_two_thousand_groups_twice_and_a_slice(lib):
    p, t, bitmap, words, (sel, chosen, sums) = large_case()
    assert t["group"][7, :3].tolist() == [5, 1024, 1024] and dd.pitch_words(1024) == 33 and (t["group"][7, 4:9] == dd.KIND_BITMAP).all()
    assert len(set(sel.tolist())) >= 7 and (words[t["cage_start"][7]:t["cage_start"][8]] != 0).sum() > 50
    first = launches(t)
    for got, want in zip(first, (bitmap, words, sel, chosen, sums)):
        assert got.view(want.dtype).tobytes() == want.tobytes()
    for got, again in zip(first, launches(t)):              # nothing depends on the order of the atomics
        assert got.tobytes() == again.tobytes()
    # slices: rings 100 .. 899 only (the other bitmaps stay zero), cages 5000 .. 14999, groups 500 .. 1499
    r, c, g = slice(100, 900), slice(5000, 15000), slice(500, 1500)
    b2, w2, s2, ch2, sm2 = launches(t, r, c, g)
    want_b = dd.fill_numpy(t["ring_xy"], t["ring_start"][100:901], t["ring_frame"][100:900], t["bitmap_words"])
    assert b2.view(np.uint32).tobytes() == want_b.tobytes() and (want_b != bitmap).any()
    want_w = dd.sets_numpy(t["group"], t["cage"][c], want_b)
    assert w2.view(np.uint32).tobytes() == want_w.tobytes()
    full = np.zeros(t["cage"].shape[0], np.uint32)
    full[c] = want_w
    want_s = dd.select_numpy(t["group"][g], t["cage_start"][500:1501], t["cage"], full, t["area"], t["random_order"][g])
    assert t["cage_start"][500] > 0 and s2.tobytes() == want_s[0].tobytes() and ch2.tobytes() == want_s[1].tobytes() and sm2.tobytes() == want_s[2].tobytes()
    # and the whole route, chunked by the byte budget
    got = dd.selections_gpu(p, 1 << 20)
    assert (got["bits"][t["rows"]] == sel).all() and got["chosen"].tobytes() == chosen.tobytes() and got["sums"].tobytes() == sums.tobytes()


def test_the_launchers_refuse_by_arguments_alone(lib):
    """No launch: every device pointer is null.  A call the checks let through ends at the null pointer check."""
    i32 = lambda a, shape: np.ascontiguousarray(np.asarray(a, np.int32).reshape(shape))
    group = lambda n=2, w=40, h=24, kinds=(1, 2), words=(0, 0): i32([n, w, h, 0, *kinds, *[0] * (5 - len(kinds)), *words, *[0] * (5 - len(words)), 0, 0], (1, 16))

    def fill(start, frames, V, words, R=None):
        s, f = i32(start, (-1,)), i32(frames, (-1, 4))
        return lib.aq_dedup_fill_u32(None, V, None, s.ctypes.data, None, f.ctypes.data, f.shape[0] if R is None else R, None, words, None), lib.aq_last_error()

    def sets(g, G=1, C=1, words=48):
        return lib.aq_dedup_sets_u32(None, g.ctypes.data, G, None, C, None, words, None, None), lib.aq_last_error()

    def select(g, start, G=1, C=4):
        s = i32(start, (-1,))
        return lib.aq_dedup_select_f64(None, g.ctypes.data, None, s.ctypes.data, G, None, None, None, C, None, None, None, None, None), lib.aq_last_error()

    through = b"null pointer"
    for (rc, msg), text in ((fill([0, 5], [[0, 40, 24, 0]], 5, 48), through),
                            (fill([0, 5], [[0, 40, 24, 0]], 5, 47), b"does not fit 47 words"),          # a bitmap array too small for its frame
                            (fill([0, 5], [[1, 40, 24, 0]], 5, 48), b"does not fit 48 words"),
                            (fill([0, 5, 10], [[0, 40, 24, 0], [24, 40, 24, 0]], 10, 71), b"the bitmap of ring 1 (24 rows of 2 words from word 24) does not fit 71 words"),
                            (fill([0, 5, 3], [[0, 40, 24, 0], [48, 40, 24, 0]], 5, 96), b"ring_start decreases at ring 1"),
                            (fill([0, 6], [[0, 40, 24, 0]], 5, 48), b"ring_start runs from 0 to 6 with 5 vertices"),
                            (fill([-1, 5], [[0, 40, 24, 0]], 5, 48), b"ring_start runs from -1"),
                            (fill([0, 5], [[0, 0, 24, 0]], 5, 48), b"frame of 0 x 24"),
                            (fill([0, 5], [[0, 40, 32769, 0]], 5, 1 << 20), b"frame of 40 x 32769"),
                            (fill([0, 5], [[0, 40, 24, 0]], 1 << 31, 48), b"2147483648 ring vertices"),
                            (fill([0, 5], [[0, 40, 24, 0]], 5, 48, R=1 << 31), b"2147483648 rings"),
                            (fill([0, 5], [[0, 40, 24, 0]], 5, 1 << 31), b"bitmap of 2147483648 words"),
                            (fill([0, 5], [[0, 40, 24, 0]], -1, 48), b"-1 ring vertices"),
                            (fill([0, 5], [[0, 40, 32768, 0]], (1 << 31) - 1, (1 << 31) - 1), through),        # the limits themselves
                            (sets(group(w=1 << 15, h=1), C=(1 << 31) - 1, words=(1 << 31) - 1), through),
                            (select(group(), [0, 4], C=(1 << 31) - 1), through),
                            (sets(group()), through),
                            (sets(group(n=6)), b"group 0 has 6 images (1 to 5"),
                            (sets(group(n=0)), b"group 0 has 0 images"),
                            (sets(group(kinds=(1, 3))), b"slot 1 of group 0 has kind 3"),
                            (sets(group(words=(0, 1))), b"ends at word 49 of 48"),
                            (sets(group(words=(0, -1))), b"the bitmap of slot 1"),
                            (sets(group(w=1 << 16)), b"frame of 65536 x 24"),
                            (sets(group(), G=1 << 31), b"2147483648 groups"),
                            (sets(group(), C=1 << 31), b"2147483648 cages"),
                            (sets(group(), words=1 << 31), b"bitmap of 2147483648 words"),
                            (select(group(), [0, 4]), through),
                            (select(group(n=6), [0, 4]), b"group 0 has 6 images"),
                            (select(group(), [0, 5]), b"cage_start runs from 0 to 5 with 4 cages"),
                            (select(group(), [-1, 4]), b"cage_start runs from -1"),
                            (select(np.concatenate([group(), group()]), [0, 3, 2], G=2), b"cage_start decreases at group 1"),
                            (select(group(), [0, 4], G=1 << 31), b"2147483648 groups"),
                            (select(group(), [0, 4], C=1 << 31), b"2147483648 cages")):
        assert rc != 0 and msg.startswith(b"dedup:") and text in msg, (text, msg)
    assert fill([0], np.zeros((0, 4)), 0, 0)[0] == 0 and sets(group(), C=0)[0] == 0 and select(group(), [0], G=0)[0] == 0      # nothing to do
    # the bindings check what they are given, and the library's refusal comes back as an error
    z = lambda shape, dt=torch.int32: torch.zeros(shape, dtype=dt, device="cuda")
    with pytest.raises(ValueError, match="contiguous CUDA"):
        engine.dedup_sets(z((1, 16), torch.int64), z((1, 8)), z(48), group())
    with pytest.raises(RuntimeError, match="dedup: group 0 has 6 images"):
        engine.dedup_sets(torch.from_numpy(group(n=6)).cuda(), z((1, 8)), z(48), group(n=6))
    with pytest.raises(RuntimeError, match="dedup: ring_start decreases"):
        engine.dedup_fill(z((10, 2)), z(3), z((2, 4)), z(96), [0, 5, 3], [[0, 40, 24, 0], [48, 40, 24, 0]])


# ---- the command lines ----

def cpu_route(tmp_path, labels, csv_path, key, geom, name, *extra):
    assert dd.main(["--labels", labels, "--geocode-bboxes", csv_path, "--blank-key", key, "--blank-geom", geom, "--out", str(tmp_path / name), "--cpu", *extra]) == 0
    return tmp_path / name


def same_files(a, b):
    for f in (dd.CAGES_FILE, dd.TILES_FILE):
        assert open(a / f, "rb").read() == open(b / f, "rb").read(), f
    da, db = json.load(open(a / dd.JSON_FILE)), json.load(open(b / dd.JSON_FILE))
    assert {k: v for k, v in da.items() if k not in ("device", "cpu")} == {k: v for k, v in db.items() if k not in ("device", "cpu")}
    return da


def test_command_line_writes_the_cpu_runs_bytes(lib, tmp_path):
    from test_dedup import COMPLETE_STATS, PARTLY_STATS, STEM, write_geom, write_key
    row = lambda cls, px, py, w, conf: f"{cls} {px / 1024:g} {py / 1024:g} {w / 1024:g} {w / 1024:g} {conf:g}\n"
    labels, csv_path = synthetic_sweep(tmp_path, (2013, 2014, 2015, 2017), {2014: [row(0, 800, 500, 10, 0.9)], 2015: [row(1, 700, 100, 30, 0.8)]})
    key = write_key(tmp_path / "key.csv", [(STEM.format(2013), PARTLY_STATS), (STEM.format(2014), PARTLY_STATS), (STEM.format(2015), COMPLETE_STATS),
                                           (STEM.format(2017), COMPLETE_STATS)])
    geom = write_geom(tmp_path / "geom.geojson", {STEM.format(2014): [(0, 0), (512, 0), (512, 1024), (0, 1024), (0, 0)],
                                                  STEM.format(2013): [(100, 0), (1024, 0), (1024, 505), (100, 505), (100, 0)]})
    for sel in ("random", "max"):
        r = subprocess.run([sys.executable, "-m", "aquaculture_amd.dedup", "--labels", labels, "--geocode-bboxes", csv_path, "--blank-key", key,
                            "--blank-geom", geom, "--out", str(tmp_path / ("gpu_" + sel)), "--dedup-selection", sel, "--dedup-seed", "5"],
                           cwd=ROOT, capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stderr[-3000:]
        doc = same_files(tmp_path / ("gpu_" + sel), cpu_route(tmp_path, labels, csv_path, key, geom, "cpu_" + sel, "--dedup-selection", sel, "--dedup-seed", "5"))
        assert doc["cages"] == 26 and doc["groups"] == 2 and doc["images_in_groups"] == 4 and 6 <= doc["survivors"]["min"] < doc["survivors"]["max"] < 20
        assert "cages on 4 images of 2 tiles" in r.stdout, r.stdout


def test_detect_py_dedups_the_years_of_its_own_sweep(lib, tmp_path):
    """A tiny sweep: four synthetic tiles in 2014 and again in 2015 (the same pass), one of them once more in 2013 with its right part white,
    one in 2017.  The three dedup files, the facility file and the tonnage files equal what the --cpu route makes of the run's label files,
    blank key and outlines."""
    from PIL import Image
    from test_tonnage import write
    from aquaculture_amd import checkpoint, facilities, geocode, tiles, tonnage as tn
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
    factors = write(tmp_path / "factors.csv", "pass,s_mean,s_sd,h_mean,h_sd\n2013-2015,12,3,0.8,0.1\n2016-2018,12,3,0.8,0.1\n")
    conf = ["--facilities-conf", "0.25", "--facilities-eps", "25", "--facilities-min-cages", "4"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "yolov5", "detect.py"), "--weights", str(tmp_path / "synth.pt"), "--source",
                        str(tmp_path / "jpegs"), "--save-txt", "--save-conf", "--nosave", "--project", str(tmp_path / "runs"), "--name", "dd",
                        "--batch-size", "4", "--geocode-bboxes", csv_path, *conf, "--facilities-by", "pass", "--facilities", "--tonnage",
                        "--tonnage-factors", factors, "--tonnage-K", "200", "--dedup-years", "--dedup-selection", "max", "--dedup-seed", "3"],
                       capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    run = tmp_path / "runs" / "dd"
    labels, key, geom = str(run / "labels"), str(run / "image_boxes_blank_key.csv"), str(run / "image_boxes_partly_blank.geojson")
    assert os.path.exists(key) and os.path.exists(geom) and "dedup years:" in r.stdout
    doc = same_files(run, cpu_route(tmp_path, labels, csv_path, key, geom, "want", *conf[:2], "--dedup-selection", "max", "--dedup-seed", "3",
                                    "--image-size", "640", "640"))
    assert doc["selection"] == "max" and doc["seed"] == 3 and doc["cages"] > 0 and doc["survivors"]["max"] < doc["cages"]
    assert max(len(row.split(",")[2].split()) for row in open(run / dd.TILES_FILE).read().splitlines()[1:]) >= 2
    table = geocode.geocode_label_dir(labels, csv_path)
    res = dd.dedup_from_table(table, key, geom, None, "max", 3, 0.25, None, 640, 640, cpu=True)
    fac = facilities.facilities_from_table(table, str(tmp_path / "want.geojson"), "pass", 0.25, 25.0, 4, 640, 640, cpu=True, dedup=res)
    got = json.load(open(run / "facilities.geojson"))
    assert got == json.load(open(tmp_path / "want.geojson")) and len(got["features"]) == len(fac["facility_index"])
    assert all("cage_ids_min" in f["properties"] and "cage_ids_max" in f["properties"] for f in got["features"])
    tn.tonnage_from_table(table, str(tmp_path / "want_t"), factors, K=200, conf_thresh=0.25, eps=25.0, min_cages=4, widths=640, heights=640, cpu=True, dedup=res)
    for f in (tn.ESTIMATES_FILE, tn.FACILITIES_FILE):
        assert open(run / f, "rb").read() == open(tmp_path / "want_t" / f, "rb").read(), f
    assert "dedup" not in open(run / "run_params.json").read()
