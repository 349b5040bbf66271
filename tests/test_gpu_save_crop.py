"""--save-crop on the MI355X: the crop encode kernel (aq_crop_jpeg_coefs) against the numpy restatement of libjpeg's pixel path, files
byte-identical to Pillow's quality=95 4:4:4 encoding, and detect.py --save-crop end to end [UPSTREAM utils/plots.py save_one_box]."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from test_save_crop import pillow_bytes, reference_coefs, torch_save_one_box_rect

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILES = [0, 1, 2, 3, 19, 20, 21, 22, 23, 24]
SIZES = [(1024, 1024), (37, 53), (300, 211), (8, 8), (1, 1), (640, 480)]


@pytest.fixture(scope="module")
def images():
    """Random uint8 RGB images of several sizes back to back in one device buffer: (device buffer, [(base, h, w, host array)])."""
    import torch
    rng = np.random.default_rng(0)
    host, parts, base = [], [], 0
    for h, w in SIZES:
        im = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        im[: h // 3] = im[: h // 3] // 64 * 64                    # some flat areas and long zero runs as well
        host.append(im.reshape(-1))
        parts.append((base, h, w, im))
        base += im.size
    return torch.from_numpy(np.concatenate(host)).cuda(), parts


def _rects(h, w, rng):
    r = [(0, 0, w, h), (0, 0, 1, 1), (w - 1, h - 1, w, h), (0, h - 1, 1, h), (w - 1, 0, w, 1)]        # full image, single pixels at the corners
    for _ in range(6):                                           # non-multiples of 8 touching each edge, and anywhere
        x1, x2 = np.sort(rng.integers(0, w + 1, 2))
        y1, y2 = np.sort(rng.integers(0, h + 1, 2))
        x2, y2 = max(x2, x1 + 1), max(y2, y1 + 1)
        if x2 > w:
            x1, x2 = w - 1, w
        if y2 > h:
            y1, y2 = h - 1, h
        r += [(x1, y1, x2, y2), (0, y1, x2, y2), (x1, 0, x2, y2), (x1, y1, w, y2), (x1, y1, x2, h)]
    return r


@pytest.fixture(scope="module")
def crops(images):
    from aquaculture_amd import engine
    _, parts = images
    rng = np.random.default_rng(1)
    bases, pitches, rects, wins = [], [], [], []
    for base, h, w, im in parts:
        for x1, y1, x2, y2 in _rects(h, w, rng):
            bases.append(base)
            pitches.append(3 * w)
            rects.append((x1, y1, x2, y2))
            wins.append(im[y1:y2, x1:x2])
    return engine.crop_table(np.asarray(bases), np.asarray(pitches), np.asarray(rects)), wins


def _check_coefs(coef, table, wins):
    for i, win in enumerate(wins):
        b = int(table["block"][i])
        want = reference_coefs(win).reshape(-1, 192)
        assert np.array_equal(coef[b:b + want.shape[0]], want), (i, win.shape)


def test_kernel_coefficients_equal_the_restatement(lib, images, crops):
    from aquaculture_amd import engine
    buf, _ = images
    table, wins = crops
    coef, t2 = engine.encode_crops(buf, table)
    assert np.array_equal(t2, table) and coef.shape[0] == int(engine.crop_blocks(table).sum())
    _check_coefs(coef, table, wins)


def test_files_equal_pillow_and_pieces_change_nothing(lib, images, crops, tmp_path):
    """The whole encoder, file for file; then the same crops through arenas too small for one piece (the largest crop alone, and 50 block
    positions without the 1024 x 1024 crop): the same coefficients, so the same bytes."""
    from aquaculture_amd import engine
    buf, _ = images
    table, wins = crops
    coef, _ = engine.encode_crops(buf, table)
    rel = [f"crops/c{i % 4}/t{i}.jpg" for i in range(len(wins))]
    assert engine.write_crop_files(str(tmp_path), rel, coef, table, threads=8) == len(wins)
    for i, win in enumerate(wins):
        assert (tmp_path / rel[i]).read_bytes() == pillow_bytes(win), (i, win.shape)
    nb = engine.crop_blocks(table)
    small, _ = engine.encode_crops(buf, table, arena_blocks=int(nb.max()))
    assert np.array_equal(small, coef)
    keep = np.nonzero(nb <= 50)[0]
    sub = engine.crop_table(table["base"][keep], table["pitch"][keep], np.stack([table[k][keep] for k in ("x1", "y1", "x2", "y2")], 1))
    tiny, _ = engine.encode_crops(buf, sub, arena_blocks=50)
    assert int(engine.crop_blocks(sub).sum()) > 4 * 50
    _check_coefs(tiny, sub, [wins[k] for k in keep])
    with pytest.raises(ValueError):
        engine.encode_crops(buf, table, arena_blocks=int(nb.max()) - 1)
    bad = table[:1].copy()
    bad["y2"] = bad["y2"] + 1                                     # one row past the buffer's first image ... and past the buffer for the last
    bad["base"] = buf.numel() - 3 * int(bad["x2"][0])
    with pytest.raises(ValueError):
        engine.encode_crops(buf, bad)


# ---- detect.py --save-crop ----

@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    from aquaculture_amd import checkpoint, tiles
    d = tmp_path_factory.mktemp("crop_cli")
    tiles.write_synthetic_jpegs(str(d / "jpegs"), TILES, size=640)
    checkpoint.write_synthetic_checkpoint(str(d / "multilabel_farms_synth.pt"), "yolov5m", 5)
    return d


def _run(workdir, name, extra=(), source=None):
    cmd = [sys.executable, os.path.join(ROOT, "yolov5", "detect.py"), "--weights", str(workdir / "multilabel_farms_synth.pt"),
           "--source", str(source or workdir / "jpegs"), "--nosave", "--save-txt", "--save-conf", "--project", str(workdir / "runs"),
           "--name", name, "--batch-size", "4", *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return workdir / "runs" / name


def _tree(d):
    out = {}
    for root, _, files in os.walk(d):
        for f in files:
            p = os.path.join(root, f)
            out[os.path.relpath(p, d)] = open(p, "rb").read()
    return out


@pytest.fixture(scope="module")
def split_run(workdir, lib):
    return _run(workdir, "crop_split", ("--save-crop", "--jpeg-decode", "split"))


def test_cli_crops_are_upstreams(workdir, split_run):
    """The crop paths are exactly those upstream's loop names for the engine's detections (in-process Engine.infer on the same batches of
    the Pillow-decoded tiles, the literal torch geometry), and every file is Pillow's encoding of that window of the decoded tile."""
    import torch
    from aquaculture_amd import checkpoint, dataloader, postprocess, tiles
    from aquaculture_amd.engine import Engine, letterbox_device
    ck = checkpoint.load_checkpoint(str(workdir / "multilabel_farms_synth.pt"))
    eng = Engine(ck, "fp32", 0)
    names = sorted(os.listdir(workdir / "jpegs"))
    want = {}
    for s in range(0, len(names), 4):
        ims = [dataloader.read_rgb(str(workdir / "jpegs" / n)) for n in names[s:s + 4]]
        x = letterbox_device(torch.from_numpy(np.stack(ims)).cuda(), (640, 640), 32, True)
        dets, counts = eng.infer(x, 0.25, 0.45, 1000)
        dets, counts = dets.cpu().numpy(), counts.cpu().numpy()
        for b, n in enumerate(names[s:s + 4]):
            seen = {}
            for row in dets[b, :counts[b]][::-1]:                 # for *xyxy, conf, cls in reversed(det)
                xyxy = np.rint(postprocess.scale_boxes((640, 640), row[None, :4], ims[b].shape[:2])).astype(np.float32)
                x1, y1, x2, y2 = torch_save_one_box_rect(xyxy, ims[b].shape[:2])[0]
                c = ck.names[int(row[5])]
                seen[c] = seen.get(c, 0) + 1
                stem = n.rsplit(".", 1)[0]
                want[f"{c}/{stem}{seen[c] if seen[c] > 1 else ''}.jpg"] = ims[b][y1:y2, x1:x2]
    eng.close()
    got = _tree(split_run / "crops")
    assert len(want) > 100 and set(got) == set(want)
    for k, win in want.items():
        assert got[k] == pillow_bytes(win), k


def test_cli_decode_paths_give_identical_crop_trees(workdir, split_run):
    ref = _tree(split_run / "crops")
    for name, extra in (("crop_host", ("--jpeg-decode", "host", "--quiet")), ("crop_gpu", ("--jpeg-decode", "gpu", "--quiet"))):
        assert _tree(_run(workdir, name, ("--save-crop", *extra)) / "crops") == ref, name


def test_cli_labels_unchanged_and_no_crops_without_the_flag(workdir, split_run):
    plain = _run(workdir, "nocrop", ("--jpeg-decode", "split"))
    assert not (plain / "crops").exists()
    assert _tree(plain / "labels") == _tree(split_run / "labels")
    import json
    assert "save_crop" not in json.load(open(plain / "run_params.json"))
    assert json.load(open(split_run / "run_params.json"))["save_crop"] is True


def test_cli_resume_does_not_duplicate_crops(workdir, split_run):
    """A finished tile that is processed again (its manifest line removed) overwrites its crops: computed names, not probed ones."""
    run = workdir / "runs" / "crop_resume"
    shutil.copytree(split_run, run)
    before = _tree(run / "crops")
    stems = open(run / "done.rank0.txt").read().split()
    again = next(s for s in stems if any(os.path.basename(k).startswith(s) for k in before))
    with open(run / "done.rank0.txt", "w") as f:
        f.write("".join(s + "\n" for s in stems if s != again))
    _run(workdir, "crop_resume", ("--save-crop", "--jpeg-decode", "split", "--resume"))
    assert _tree(run / "crops") == before
    assert sorted(open(run / "done.rank0.txt").read().split()) == sorted(stems)


def test_cli_scene_mode_crops_equal_the_tile_sweep(tmp_path, lib):
    """--tile-scenes: crops cut from the raster on the device equal those of the ordinary sweep over the same tiles stored losslessly."""
    from PIL import Image
    from aquaculture_amd import checkpoint, scenes, tiles
    checkpoint.write_synthetic_checkpoint(str(tmp_path / "multilabel_farms_synth.pt"), "yolov5m", 5)
    scene = np.zeros((1500, 2048, 3), np.uint8)
    for (x0, y0), i in {(0, 0): 19, (1024, 0): 3, (0, 1024): 20, (1024, 1024): 19}.items():
        scene[y0:y0 + 1024, x0:x0 + 1024] = tiles.synthetic_tile(i, 1024)[: min(1024, 1500 - y0)]
    (tmp_path / "scenes").mkdir()
    (tmp_path / "pngs").mkdir()
    spath = tmp_path / "scenes" / "ORTHOIMAGERY.ORTHOPHOTOS2015_7.tif"
    Image.fromarray(scene).save(spath)
    for x0, y0, w, h in scenes.tile_grid(2048, 1500):
        Image.fromarray(scene[y0:y0 + h, x0:x0 + w]).save(tmp_path / "pngs" / (scenes.tile_stem(str(spath), x0, y0) + ".png"))
    ref = _tree(_run(tmp_path, "tiles", ("--save-crop", "--quiet"), source=tmp_path / "pngs") / "crops")
    got = _tree(_run(tmp_path, "scene", ("--save-crop", "--tile-scenes"), source=tmp_path / "scenes") / "crops")
    assert len(ref) > 50 and got == ref
