"""--blank-geom on the GPU: aq_blank_components_u8 and aq_blank_ring_edges_u8 against blank_geom.components_numpy (records, both label maps,
the winner's outer edges), and the GeoJSON file detect.py writes against what blank_geom computes from Pillow's decode of the same files.
Every CLI step runs in a child process under its own time limit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_blank_geom import MASKS, constructed_masks, image_of

from aquaculture_amd import blank, blank_geom

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKIPPED = lambda h, w: [0, 0, -1, 0, 0, w, h, -1, -1, 0, 0, 0]          # noqa: E731  (the record of a frame that was not examined)


def _pack(images, bases=None, pitches=None, fill=7):
    """Images into one host buffer at the given byte offsets and row pitches (default: back to back) -> (uint8 buffer, bases, pitches)."""
    pitches = [3 * im.shape[1] if p is None else p for im, p in zip(images, pitches or [None] * len(images))]
    if bases is None:
        bases, at = [], 0
        for im, p in zip(images, pitches):
            bases.append(at)
            at += (im.shape[0] - 1) * p + 3 * im.shape[1]
    end = max(b + (im.shape[0] - 1) * p + 3 * im.shape[1] for im, b, p in zip(images, bases, pitches))
    buf = np.full(end + 5, fill, np.uint8)
    for im, b, p in zip(images, bases, pitches):
        for y in range(im.shape[0]):
            buf[b + y * p: b + y * p + 3 * im.shape[1]] = im[y].reshape(-1)
    return buf, bases, pitches


def _gpu(buf, images, bases, pitches, stats_dev=None, labels=True):
    """-> (records [n, 12], per image (fg map, bg map) or None, per image edges, table, device buffer)"""
    from aquaculture_amd.engine import blank_components, blank_geom_frame_table, blank_ring_edges
    table = blank_geom_frame_table(np.asarray(bases, np.int64), np.asarray(pitches, np.int64), [im.shape[:2] for im in images])
    dev = torch.from_numpy(buf).cuda() if isinstance(buf, np.ndarray) else buf
    got = blank_components(dev, table, stats_dev=stats_dev, labels=labels)
    rec_dev, scratch, table_dev = got[:3]
    torch.cuda.synchronize()
    rec = rec_dev.cpu().numpy()
    maps = None
    if labels:
        flat = got[3].cpu().numpy()
        maps = []
        for f in table:
            h, w, at = int(f["h"]), int(f["w"]), 2 * int(f["mcu"])
            maps.append((flat[at: at + h * w].reshape(h, w), flat[at + h * w: at + 2 * h * w].reshape(h, w)))
    edges = blank_ring_edges(table, rec, rec_dev, scratch, table_dev)
    return rec, maps, edges, table, dev


def _check(rec, maps, edges, images, examined=None, want=None):
    assert rec.dtype == np.int32 and rec.shape == (len(images), 12)
    for k, im in enumerate(images):
        h, w = im.shape[:2]
        if examined is not None and not examined[k]:
            assert rec[k].tolist() == SKIPPED(h, w) and edges[k].shape == (0, 2), (k, rec[k].tolist())
            continue
        c = want[k] if want is not None else blank_geom.components_numpy(im)
        assert rec[k].tolist() == c["record"].tolist(), (k, im.shape, dict(zip(blank_geom.RECORD_FIELDS, rec[k].tolist())),
                                                         dict(zip(blank_geom.RECORD_FIELDS, c["record"].tolist())))
        if maps is not None:
            assert (maps[k][0] == c["fg"]).all() and (maps[k][1] == c["bg"]).all(), (k, im.shape)
        assert edges[k].dtype == np.int32 and edges[k].tolist() == c["edges"].tolist(), (k, im.shape)
        if c["record"][1]:
            assert blank_geom.ring_area(blank_geom.ring_from_edges(edges[k], w)) == rec[k][4]


def test_constructed_and_random_cases_in_one_buffer_of_mixed_sizes(lib):
    images = [image_of(m, k) for k, (_, m) in enumerate(MASKS)]
    buf, bases, pitches = _pack(images)
    rec, maps, edges, _, _ = _gpu(buf, images, bases, pitches)
    _check(rec, maps, edges, images)
    assert len(constructed_masks()) >= 10 and {0, 1}.issubset(set(rec[:, 1].tolist()))


@pytest.mark.parametrize("w", [1, 15, 63, 64, 65, 1000, 1024, 2500])
def test_widths_odd_bases_and_pitches(lib, w):
    rng = np.random.Generator(np.random.PCG64(200 + w))
    images = []
    for k, h in enumerate((1, 33, 70)):
        density = (0.5, 0.62, 0.9)[k]
        m = rng.random((h, w)) < density
        if k == 2:
            m[h // 2:, w // 3: w // 3 + 2] = False          # cuts, so that the largest region is not simply everything
            m[h // 3] = False
        images.append(image_of(m, 7 * w + k))
    pitches = [3 * w, 3 * w + 1, 3 * w + 13]
    bases, at = [], 3
    for im, p in zip(images, pitches):
        bases.append(at)
        at += (im.shape[0] - 1) * p + 3 * w + 5
    buf, bases, pitches = _pack(images, bases, pitches, fill=0)
    rec, maps, edges, _, _ = _gpu(buf, images, bases, pitches)
    _check(rec, maps, edges, images)


def test_windows_of_a_larger_raster(lib):
    rng = np.random.Generator(np.random.PCG64(6))
    coarse = rng.random((35, 75)) < 0.6
    m = np.kron(coarse, np.ones((20, 20), bool)).astype(bool) & (rng.random((700, 1500)) < 0.995)
    m[:, 1300:] = False                                     # a white margin, as the edge of a scene has
    m[650:] = False
    raster = image_of(m, 9)
    wins = [(0, 0, 512, 512), (512, 0, 512, 512), (1024, 0, 476, 512), (1024, 512, 476, 188), (3, 5, 1001, 333)]
    images = [np.ascontiguousarray(raster[y:y + h, x:x + w]) for x, y, w, h in wins]
    bases = [y * 4500 + 3 * x for x, y, w, h in wins]
    rec, maps, edges, _, _ = _gpu(raster.reshape(-1).copy(), images, bases, [4500] * len(wins))
    _check(rec, maps, edges, images)


def _tile_masks(n=64, size=1024):
    """Masks of n tiles: blobs of 64-px blocks with pinholes, white bands on every fourth, two tiles of pixel noise, one empty, one full."""
    rng = np.random.Generator(np.random.PCG64(12))
    out = []
    for k in range(n):
        if k in (5, 6):
            m = rng.random((size, size)) < (0.45, 0.7)[k - 5]
        elif k == 1:
            m = np.zeros((size, size), bool)
        elif k == 2:
            m = np.ones((size, size), bool)
        else:
            m = np.kron(rng.random((16, 16)) < 0.6, np.ones((size // 16, size // 16), bool)).astype(bool)
            m &= rng.random((size, size)) < 0.9995
        if k % 4 == 0:
            m[:100] = False
            m[:, size - 37:] = False
        out.append(m)
    return out


def test_64_tiles_of_1024_px_skipped_frames_and_two_calls_give_the_same_bytes(lib):
    from aquaculture_amd.engine import blank_components, blank_frame_table, blank_stats
    masks = _tile_masks()
    images = [image_of(m, 100 + k) for k, m in enumerate(masks)]
    for k in range(0, 64, 4):                               # the bands are white, so that the key calls these tiles partly blank
        images[k][:100] = 255
        images[k][:, 1024 - 37:] = 255
    images[3] = np.full((1024, 1024, 3), 255, np.uint8)     # blank by its grey levels
    masks[3] = np.zeros((1024, 1024), bool)
    tiles = torch.from_numpy(np.stack(images)).cuda()
    bases = [k * 1024 * 1024 * 3 for k in range(64)]
    want = [blank_geom.components_numpy(mask=m) for m in masks]
    rec, maps, edges, table, dev = _gpu(tiles.view(-1), images, bases, [3072] * 64)
    _check(rec, maps, edges, images, want=want)
    assert rec[1].tolist() == [1, 0, -1, 0, 0, 1024, 1024, -1, -1, 0, 0, 0] and rec[2][1:5].tolist() == [1, 0, 1 << 20, 1 << 20]
    again = blank_components(dev, table)[0]
    torch.cuda.synchronize()
    assert again.cpu().numpy().tobytes() == rec.tobytes()
    # with the key's records: only partly blank frames with a non-blank pixel are examined
    stats = blank_stats(dev, blank_frame_table(np.asarray(bases, np.int64), 3072, [(1024, 1024)] * 64))
    torch.cuda.synchronize()
    st = stats.cpu().numpy()
    examined = [s == "partly blank" and int(r[4]) > 0 for s, r in zip(blank.status(st), st)]
    assert {"blank", "partly blank", "complete"} == set(blank.status(st)) and 8 <= sum(examined) < 64 and not examined[3]
    rec2, _, edges2, _, _ = _gpu(dev, images, bases, [3072] * 64, stats_dev=stats.contiguous(), labels=False)
    _check(rec2, None, edges2, images, examined=examined, want=want)


def test_refused_tables_launch_nothing(lib):
    from aquaculture_amd.engine import blank_components, blank_geom_frame_table, blank_ring_edges, load_library
    dev = torch.zeros(64 * 64 * 3, dtype=torch.uint8, device="cuda")
    out = torch.full((2, 12), -77, dtype=torch.int32, device="cuda")
    table = blank_geom_frame_table(np.asarray([0, 64 * 32 * 3], np.int64), 192, [(32, 64), (33, 64)])       # the second one ends a row too late
    need = int(load_library().aq_blank_geom_scratch_bytes(table.ctypes.data, 2))
    assert need == 2 * 64 + 9 * int(table["mcu"][1] + (65 * 33 + 2 + 3) // 4 * 4)
    scratch = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="frame 1 .*leaves its buffer"):
        blank_components(dev, table, scratch=scratch, out=out)
    bad = table.copy()
    bad["h"][1], bad["mcu"][1] = 32, 7                      # a scratch part that would overlap the first frame's
    with pytest.raises(RuntimeError, match="scratch at slot"):
        blank_components(dev, bad, scratch=scratch, out=out)
    good = blank_geom_frame_table(np.asarray([0, 64 * 32 * 3], np.int64), 192, [(32, 64), (32, 64)])
    lib_ = load_library()
    good_dev = torch.from_numpy(good.view(np.uint8).copy()).cuda()          # (a real table: a call that went ahead would read it)
    need_good = int(lib_.aq_blank_geom_scratch_bytes(good.ctypes.data, 2))
    assert need_good == 2 * 64 + 9 * 2 * (65 * 32 + 4) <= need
    rc = lib_.aq_blank_components_u8(dev.data_ptr(), dev.numel(), good_dev.data_ptr(), good.ctypes.data, 2, None, scratch.data_ptr(), need_good - 1,
                                     out.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
    assert rc != 0 and b"bytes of scratch" in lib_.aq_last_error()
    assert blank_components(dev, table[:0], scratch=scratch, out=out)[0].shape == (0, 12)      # no frames: a no-op
    torch.cuda.synchronize()
    assert bool((out == -77).all()) and bool((scratch == 0x5A).all())
    # the edges call: slices that do not fit their buffer
    rec_dev, scratch2, table_dev = blank_components(dev + 1, good)
    rec = rec_dev.cpu().numpy()
    assert rec[:, 1].tolist() == [1, 1] and rec[:, 10].tolist() == [2 * 64 + 2 * 30] * 2
    at = np.asarray([0, 188, 376], np.int64)
    edges = torch.full((376, 2), -5, dtype=torch.int32, device="cuda")
    rc = lib_.aq_blank_ring_edges_u8(table_dev.data_ptr(), good.ctypes.data, 2, scratch2.data_ptr(), scratch2.numel(), rec_dev.data_ptr(),
                                     torch.from_numpy(at).cuda().data_ptr(), at.ctypes.data, edges.data_ptr(), 375, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc != 0 and b"room for 375" in lib_.aq_last_error() and bool((edges == -5).all())
    got = blank_ring_edges(good, rec, rec_dev, scratch2, table_dev)
    assert [e.shape for e in got] == [(188, 2)] * 2 and got[0].tolist() == blank_geom.components_numpy(mask=np.ones((32, 64), bool))["edges"].tolist()


# ---- detect.py --blank-geom ----

def _constructed_tiles(size=640):
    """name -> uint8 RGB image: white bands and corners, a white frame with an island, speckle at the 250 threshold, and plain tiles."""
    from aquaculture_amd import tiles
    rng = np.random.Generator(np.random.PCG64(77))
    out = {}
    for k, i in enumerate((0, 3)):
        out[f"ORTHOIMAGERY.ORTHOPHOTOS2015_{k}_0_{1024 * k}.jpeg"] = tiles.synthetic_tile(i, size)
    out["ORTHOIMAGERY.ORTHOPHOTOS2015_7_1024_0.jpeg"] = np.full((size, size, 3), 255, np.uint8)
    im = tiles.synthetic_tile(19, size).copy()              # a white band and a white corner
    im[:, size - 160:] = 255
    im[:120, :200] = 255
    out["ORTHOIMAGERY.ORTHOPHOTOS.ORTHO-EXPRESS.2021_9_0_2048.jpeg"] = im
    im = np.full((size, size, 3), 255, np.uint8)            # a white frame around the imagery, an island in the frame, a lake in the imagery
    im[90:560, 100:500] = tiles.synthetic_tile(3, size)[90:560, 100:500]
    im[300:340, 200:260] = 255
    im[315:325, 225:235] = 40
    im[20:50, 530:600] = (60, 90, 120)
    out["ORTHOIMAGERY.ORTHOPHOTOS.ORTHO-EXPRESS.2021_9_1024_2048.jpeg"] = im
    im = tiles.synthetic_tile(20, size).copy()              # speckle: levels around 250 beside hard edges that ring in the JPEG
    im[:96] = 255
    im[96:300, 400:] = rng.integers(244, 256, (204, 240, 1))
    im[400:, :64] = 255
    im[430:600:6, 8:56:5] = 0
    out["ORTHOIMAGERY.ORTHOPHOTOS2015_3_2048_1024.jpeg"] = im
    im = np.full((size, size, 3), 255, np.uint8)            # partly blank by its averages, but no pixel below 250 in every channel
    im[200:400, 200:400] = (255, 255, 0)
    out["ORTHOIMAGERY.ORTHOPHOTOS2015_4_0_3072.jpeg"] = im
    return out


BBOXES = {k: (1000.0 + 7000.0 * k, 5000.0, 1000.0 + 7000.0 * k + 6144 * 0.2, 5000.0 + 6144 * 0.2) for k in range(10)}


@pytest.fixture(scope="module")
def workdir(tmp_path_factory, lib):
    from PIL import Image
    from aquaculture_amd import checkpoint
    d = tmp_path_factory.mktemp("blank_geom_cli")
    (d / "jpegs").mkdir()
    for name, im in _constructed_tiles().items():
        Image.fromarray(im).save(d / "jpegs" / name, quality=95)       # (4:2:0 baseline: every --jpeg-decode mode reads it)
    with open(d / "wanted_bboxes.csv", "w") as f:
        f.write(",geometry\n")
        for k, (x0, y0, x1, y1) in BBOXES.items():
            f.write(f'{k},"POLYGON (({x0} {y0}, {x1} {y0}, {x1} {y1}, {x0} {y1}, {x0} {y0}))"\n')
    checkpoint.write_synthetic_checkpoint(str(d / "multilabel_farms_synth.pt"), "yolov5m", 5)
    return d


def _file_text(tmp, names, images, table=None, tol=0.5):
    """The file blank_geom writes for these decoded images: a feature (or "actually blank") per partly blank one, in listing order."""
    tmp.mkdir(exist_ok=True)
    for old in tmp.glob("blank_geom.rank*.jsonl"):
        os.remove(old)
    part = blank_geom.PartFile(str(tmp), 0)
    part.open()
    for k, (n, im) in enumerate(zip(names, images)):
        if blank.status(blank.stats_numpy(im)) == ["partly blank"]:
            part.append([k], blank_geom.part_rows([n], [blank_geom.feature_numpy(n, im, table, tol)]))
    part.close()
    got = blank_geom.merge_parts(str(tmp), str(tmp / "want.geojson"), names, crs="urn:ogc:def:crs:EPSG::3857" if table is not None else None)
    return open(tmp / "want.geojson").read(), got["features"], got["actually_blank"]


def _summary(kept, actually_blank):
    """The two parts of detect.py's closing line about the file."""
    return (f"blank geom: {kept} polygons of partly blank images",
            f"; {len(actually_blank)} actually blank" + (": " + " ".join(actually_blank) if actually_blank else ""))


def _expected(workdir, tmp, table=None, tol=0.5, every=1):
    from aquaculture_amd import dataloader
    names = [os.path.basename(f) for f in dataloader.list_images(str(workdir / "jpegs"))][::every]
    return _file_text(tmp, names, [dataloader.read_rgb(str(workdir / "jpegs" / n)) for n in names], table, tol)


def _run(workdir, name, extra=(), source="jpegs", ok=True):
    cmd = [sys.executable, os.path.join(ROOT, "yolov5", "detect.py"), "--weights", str(workdir / "multilabel_farms_synth.pt"),
           "--source", str(workdir / source), "--save-txt", "--save-conf", "--nosave", "--project", str(workdir / "runs"),
           "--name", name, "--batch-size", "4", *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=420)
    assert (r.returncode == 0) == ok, r.stdout[-2000:] + r.stderr[-2000:]
    return (workdir / "runs" / name), r.stdout + r.stderr


def test_decoded_files_cover_the_cases(workdir, tmp_path):
    from aquaculture_amd import dataloader
    text, kept, actually_blank = _expected(workdir, tmp_path / "w")
    assert kept >= 3 and kept + len(actually_blank) == 4 and len(json.loads(text)["features"]) == kept       # (the JPEG decides about the yellow tile's edge)
    by = {f["properties"]["image"]: f["properties"] for f in json.loads(text)["features"]}
    assert by["ORTHOIMAGERY.ORTHOPHOTOS.ORTHO-EXPRESS.2021_9_1024_2048.jpeg"]["n_components"] >= 3          # imagery, island in the lake, island in the frame
    assert by["ORTHOIMAGERY.ORTHOPHOTOS2015_3_2048_1024.jpeg"]["n_components"] > 20                             # speckle
    im = dataloader.read_rgb(str(workdir / "jpegs" / "ORTHOIMAGERY.ORTHOPHOTOS2015_3_2048_1024.jpeg"))
    near = im.max(axis=2)
    assert ((near >= 245) & (near < 250)).sum() > 100 and ((near >= 250) & (near < 255)).sum() > 100


@pytest.mark.parametrize("mode", ["host", "split", "gpu"])
def test_cli_file_equals_blank_geom_on_pillows_decode_under_each_decode_mode(workdir, tmp_path, mode):
    metres = mode == "split"                                # one of the modes with the bounds table: rings in EPSG:3857, simplified
    extra = ("--geocode-bboxes", str(workdir / "wanted_bboxes.csv"), "--blank-geom-simplify", "0.3") if metres else ()
    run, out = _run(workdir, f"geom_{mode}", ("--blank-geom", "--jpeg-decode", mode) + extra)
    want, kept, actually_blank = _expected(workdir, tmp_path / "w", table=BBOXES if metres else None, tol=0.3)
    assert open(run / blank_geom.GEOM_FILE).read() == want
    assert all(part in out for part in _summary(kept, actually_blank))
    params = json.load(open(run / "run_params.json"))
    assert params["blank_geom"] is True and params["blank_key"] is True and os.path.exists(run / blank.KEY_FILE)
    doc = json.loads(want)
    assert ("crs" in doc) == metres
    if metres:
        for f in doc["features"]:
            xs = [p[0] for p in f["geometry"]["coordinates"][0]]
            x0 = BBOXES[int(f["properties"]["bbox_ind"])][0]
            assert x0 <= min(xs) and max(xs) <= x0 + 6144 * 0.2 and len(xs) <= len(f["properties"]["ring_px"])


def test_cli_without_the_flag_writes_no_file_and_a_given_path_is_used(workdir, tmp_path):
    run, out = _run(workdir, "plain", ("--blank-key",))
    assert not [f for f in os.listdir(run) if "blank_geom" in f or f.endswith(".geojson")] and "blank geom" not in out
    assert "blank_geom" not in json.load(open(run / "run_params.json"))
    run, _ = _run(workdir, "path", ("--blank-geom", str(tmp_path / "g.geojson")))
    assert open(tmp_path / "g.geojson").read() == _expected(workdir, tmp_path / "w")[0] and not os.path.exists(run / blank_geom.GEOM_FILE)


def test_cli_resume_after_half_of_the_files_gives_the_same_file(workdir, tmp_path):
    import shutil
    from aquaculture_amd import dataloader
    names = [os.path.basename(f) for f in dataloader.list_images(str(workdir / "jpegs"))]
    (workdir / "half").mkdir()
    for n in names[::2]:
        shutil.copy(workdir / "jpegs" / n, workdir / "half" / n)
    run, _ = _run(workdir, "resumed", ("--blank-geom",), source="half")
    assert open(run / blank_geom.GEOM_FILE).read() == _expected(workdir, tmp_path / "w", every=2)[0]
    for n in names[1::2]:
        shutil.copy(workdir / "jpegs" / n, workdir / "half" / n)
    run, out = _run(workdir, "resumed", ("--blank-geom", "--resume"), source="half")
    assert open(run / blank_geom.GEOM_FILE).read() == _expected(workdir, tmp_path / "w")[0]
    assert f"resume: {len(names[::2])} tiles recorded as done" in out


def test_cli_scene_mode_with_a_white_margin(tmp_path, lib):
    from PIL import Image
    from aquaculture_amd import checkpoint, scenes, tiles
    checkpoint.write_synthetic_checkpoint(str(tmp_path / "multilabel_farms_synth.pt"), "yolov5m", 5)
    scene = np.full((1500, 2048, 3), 255, np.uint8)
    scene[:1024, :1024] = tiles.synthetic_tile(19, 1024)
    scene[:1024, 1024:1800] = tiles.synthetic_tile(3, 1024)[:, :776]
    scene[1024:1300, :1024] = tiles.synthetic_tile(20, 1024)[:276]
    scene[1100:1200, 300:500] = 255                         # a lake in the third tile
    scene[1140:1150, 390:400] = 0
    scene[1100:1200, 1200:1300] = (255, 255, 0)             # the fourth tile: partly blank by its grey levels and averages, no pixel below 250
    (tmp_path / "scenes").mkdir()
    spath = tmp_path / "scenes" / "ORTHOIMAGERY.ORTHOPHOTOS2015_7.tif"
    Image.fromarray(scene).save(spath)
    grid = scenes.tile_grid(2048, 1500)
    cmd = [sys.executable, os.path.join(ROOT, "yolov5", "detect.py"), "--weights", str(tmp_path / "multilabel_farms_synth.pt"),
           "--source", str(tmp_path / "scenes"), "--tile-scenes", "--save-txt", "--save-conf", "--nosave", "--blank-geom",
           "--project", str(tmp_path / "runs"), "--name", "scene", "--batch-size", "4"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    names = [scenes.tile_stem(str(spath), x0, y0) + ".tif" for x0, y0, w, h in grid]
    images = [np.ascontiguousarray(scene[y0:y0 + h, x0:x0 + w]) for x0, y0, w, h in grid]
    want, kept, actually_blank = _file_text(tmp_path / "w", names, images)
    assert kept == 2 and actually_blank == [names[3]] and open(tmp_path / "runs" / "scene" / blank_geom.GEOM_FILE).read() == want
    assert all(part in r.stdout + r.stderr for part in _summary(kept, actually_blank))
