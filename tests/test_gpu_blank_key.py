"""--blank-key on the GPU: aq_blank_stats_u8 against blank.stats_numpy and the literal Pillow / numpy expressions, field for field, and the
key file detect.py writes.  Every CLI step runs in a child process under its own time limit."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_blank_key import CASES, literal_mask_stats, literal_status

from aquaculture_amd import blank

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def _gpu(buf, images, bases, pitches):
    from aquaculture_amd.engine import blank_frame_table, blank_stats
    table = blank_frame_table(np.asarray(bases, np.int64), np.asarray(pitches, np.int64), [im.shape[:2] for im in images])
    dev = torch.from_numpy(buf).cuda() if isinstance(buf, np.ndarray) else buf
    out = blank_stats(dev, table)
    torch.cuda.synchronize()
    return out.cpu().numpy(), table, dev


def _check(got, images):
    assert got.dtype == np.int32 and got.shape == (len(images), 9)
    for k, im in enumerate(images):
        want = blank.stats_numpy(im)
        assert got[k].tolist() == want.tolist(), (k, im.shape, dict(zip(blank.FIELDS, got[k].tolist())), dict(zip(blank.FIELDS, want.tolist())))
        st, extrema, rc = literal_status(im)
        assert blank.status(got[k]) == [st] and (int(got[k][0]), int(got[k][1])) == extrema
        if rc is not None:
            assert (int(got[k][2]), int(got[k][3])) == rc
        n, box = literal_mask_stats(im)
        assert int(got[k][4]) == n and tuple(got[k][5:].tolist()) == box


def test_branch_cases_in_one_buffer_of_mixed_sizes(lib):
    images = [im for _, im in CASES]
    buf, bases, pitches = _pack(images)
    got, _, _ = _gpu(buf, images, bases, pitches)
    _check(got, images)
    assert set(blank.status(got)) == {"blank", "partly blank", "complete"}


@pytest.mark.parametrize("w", [1, 15, 16, 17, 1000, 1024, 1040, 2500])
def test_widths_odd_bases_and_pitches(lib, w):
    rng = np.random.Generator(np.random.PCG64(100 + w))
    images = []
    for k, h in enumerate((1, 33, 70)):
        im = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        if k == 1:
            im[h // 2] = 255
            im[:, w - 1] = 252
        if k == 2:
            im[:] = rng.integers(250, 256, (h, w, 3))
            im[h - 1, w - 1] = (9, 250, 250)
        images.append(im)
    pitches = [3 * w, 3 * w + 1, 3 * w + 13]
    bases, at = [], 3
    for im, p in zip(images, pitches):
        bases.append(at)
        at += (im.shape[0] - 1) * p + 3 * w + 5
    buf, bases, pitches = _pack(images, bases, pitches, fill=255)
    got, _, _ = _gpu(buf, images, bases, pitches)
    _check(got, images)


def test_windows_of_a_larger_raster(lib):
    rng = np.random.Generator(np.random.PCG64(5))
    raster = rng.integers(0, 240, (700, 1500, 3)).astype(np.uint8)
    raster[:, 1300:] = 255                                  # a white margin, as the edge of a scene has
    raster[650:] = 255
    wins = [(0, 0, 512, 512), (512, 0, 512, 512), (1024, 0, 476, 512), (1024, 512, 476, 188), (3, 5, 1001, 333)]
    images = [np.ascontiguousarray(raster[y:y + h, x:x + w]) for x, y, w, h in wins]
    bases = [y * 4500 + 3 * x for x, y, w, h in wins]
    got, _, _ = _gpu(raster.reshape(-1).copy(), images, bases, [4500] * len(wins))
    _check(got, images)
    assert blank.status(got)[2] == "partly blank"


def test_64_tiles_of_1024_px_and_two_calls_give_the_same_bytes(lib):
    from aquaculture_amd.engine import blank_stats
    g = torch.Generator(device="cuda").manual_seed(11)
    tiles = torch.randint(0, 256, (64, 1024, 1024, 3), generator=g, device="cuda", dtype=torch.uint8)
    tiles[1] = 255
    tiles[2, :, 1000:] = 255
    tiles[3, 17] = 251
    tiles[4] = torch.randint(250, 256, (1024, 1024, 3), generator=g, device="cuda", dtype=torch.uint8)
    tiles[5].fill_(0)
    tiles[6].fill_(1)
    images = [t.cpu().numpy() for t in tiles]
    bases = [k * 1024 * 1024 * 3 for k in range(64)]
    got, table, dev = _gpu(tiles.view(-1), images, bases, [3072] * 64)
    _check(got, images)
    assert blank.status(got)[:7] == ["complete", "blank", "partly blank", "partly blank", "blank", "blank", "blank"]
    again = blank_stats(dev, table)
    torch.cuda.synchronize()
    assert again.cpu().numpy().tobytes() == got.tobytes()


def test_an_image_whose_base_lies_beyond_2_gib(lib):
    need = (1 << 31) + (64 << 20)
    free = torch.cuda.mem_get_info()[0]
    if free < need + (1 << 30):
        pytest.skip(f"needs {need >> 20} MiB of device memory, {free >> 20} MiB are free")
    rng = np.random.Generator(np.random.PCG64(31))
    far = rng.integers(0, 256, (300, 1000, 3)).astype(np.uint8)
    far[100] = 255
    near = rng.integers(0, 256, (64, 64, 3)).astype(np.uint8)
    dev = torch.zeros(need, dtype=torch.uint8, device="cuda")
    base = (1 << 31) + 12345
    dev[base: base + far.size] = torch.from_numpy(far.reshape(-1)).cuda()
    dev[: near.size] = torch.from_numpy(near.reshape(-1)).cuda()
    got, _, _ = _gpu(dev, [near, far], [0, base], [192, 3000])
    _check(got, [near, far])


def test_a_frame_that_leaves_the_buffer_is_refused_and_nothing_is_launched(lib):
    from aquaculture_amd.engine import blank_frame_table, blank_stats
    dev = torch.zeros(64 * 64 * 3, dtype=torch.uint8, device="cuda")
    out = torch.full((2, 9), -77, dtype=torch.int32, device="cuda")
    scratch = torch.full((4096,), 0x5A, dtype=torch.uint8, device="cuda")
    table = blank_frame_table(np.asarray([0, 64 * 32 * 3], np.int64), 192, [(32, 64), (33, 64)])       # the second one ends a row too late
    with pytest.raises(RuntimeError, match="frame 1 .*leaves its buffer"):
        blank_stats(dev, table, scratch=scratch, out=out)
    torch.cuda.synchronize()
    assert bool((out == -77).all()) and bool((scratch == 0x5A).all())
    bad = table.copy()
    bad["base"][1], bad["mcu"][1] = 0, 7                   # column sums that would overlap the first frame's
    with pytest.raises(RuntimeError, match="column sums"):
        blank_stats(dev, bad, scratch=scratch, out=out)
    # no frames: a no-op
    assert blank_stats(dev, table[:0], scratch=scratch, out=out).shape == (0, 9)
    torch.cuda.synchronize()
    assert bool((out == -77).all()) and bool((scratch == 0x5A).all())


# ---- detect.py --blank-key ----

def _constructed_tiles(size=640):
    """name -> (uint8 RGB image, the status it is built for)."""
    from aquaculture_amd import tiles
    out = {}
    for k, i in enumerate((0, 3, 19, 20)):
        out[f"ORTHOIMAGERY.ORTHOPHOTOS2015_{k}_0_{1024 * k}.jpeg"] = (tiles.synthetic_tile(i, size), None)
    out["ORTHOIMAGERY.ORTHOPHOTOS2015_7_1024_0.jpeg"] = (np.full((size, size, 3), 255, np.uint8), "blank")
    out["ORTHOIMAGERY.ORTHOPHOTOS2015_8_1024_0.jpeg"] = (np.zeros((size, size, 3), np.uint8), "blank")
    im = tiles.synthetic_tile(19, size).copy()
    im[:, size - 160:] = 255
    out["ORTHOIMAGERY.ORTHOPHOTOS.ORTHO-EXPRESS.2021_9_0_2048.jpeg"] = (im, "partly blank")
    im = tiles.synthetic_tile(3, size).copy()
    im[:96] = 255
    out["ORTHOIMAGERY.ORTHOPHOTOS.ORTHO-EXPRESS.2021_9_1024_2048.jpeg"] = (im, "partly blank")
    im = np.full((size, size, 3), 253, np.uint8)
    out["tile_near_white.jpeg"] = (im, "blank")
    return out


@pytest.fixture(scope="module")
def workdir(tmp_path_factory, lib):
    from PIL import Image
    from aquaculture_amd import checkpoint
    d = tmp_path_factory.mktemp("blank_cli")
    (d / "jpegs").mkdir()
    for name, (im, _) in _constructed_tiles().items():
        Image.fromarray(im).save(d / "jpegs" / name, quality=95)       # (4:2:0 baseline: every --jpeg-decode mode reads it)
    checkpoint.write_synthetic_checkpoint(str(d / "multilabel_farms_synth.pt"), "yolov5m", 5)
    return d


def _expected(workdir, source="jpegs"):
    """(names in listing order, statuses, records) from the decoded files, Pillow on the CPU."""
    from aquaculture_amd import dataloader
    names = [os.path.basename(f) for f in dataloader.list_images(str(workdir / source))]
    recs = [blank.stats_numpy(dataloader.read_rgb(str(workdir / source / n))) for n in names]
    for n, r in zip(names, recs):
        assert blank.status(r) == [literal_status(dataloader.read_rgb(str(workdir / source / n)))[0]]
    return names, [blank.status(r)[0] for r in recs], recs


def _run(workdir, name, extra=(), source="jpegs", ok=True):
    cmd = [sys.executable, os.path.join(ROOT, "yolov5", "detect.py"), "--weights", str(workdir / "multilabel_farms_synth.pt"),
           "--source", str(workdir / source), "--save-txt", "--save-conf", "--nosave", "--project", str(workdir / "runs"),
           "--name", name, "--batch-size", "4", *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=420)
    assert (r.returncode == 0) == ok, r.stdout[-2000:] + r.stderr[-2000:]
    return (workdir / "runs" / name), r.stdout + r.stderr


def _labels(run):
    return {f: open(run / "labels" / f, "rb").read() for f in sorted(os.listdir(run / "labels"))}


def _key_text(names, recs):
    return blank.HEADER + "".join(f"{i},{row}\n" for i, row in enumerate(blank.key_rows(names, np.stack(recs))))


def test_decoded_files_still_have_the_status_they_were_built_for(workdir):
    names, statuses, _ = _expected(workdir)
    built = _constructed_tiles()
    for n, st in zip(names, statuses):
        assert built[n][1] in (None, st), (n, st)
    assert set(statuses) == {"blank", "partly blank", "complete"}


@pytest.fixture(scope="module")
def plain_run(workdir):
    return _run(workdir, "plain")[0]


def test_cli_without_the_flag_writes_no_key(plain_run):
    import json
    assert not [f for f in os.listdir(plain_run) if "blank" in f]
    assert "blank_key" not in json.load(open(plain_run / "run_params.json"))


@pytest.mark.parametrize("mode", ["host", "split", "gpu"])
def test_cli_key_equals_pillow_statuses_under_each_decode_mode(workdir, plain_run, mode):
    import json
    run, out = _run(workdir, f"key_{mode}", ("--blank-key", "--jpeg-decode", mode))
    names, statuses, recs = _expected(workdir)
    text = open(run / blank.KEY_FILE).read()
    assert text == _key_text(names, recs)
    assert [line.split(",")[5] for line in text.splitlines()[1:]] == statuses
    assert _labels(run) == _labels(plain_run) and _labels(run)
    assert json.load(open(run / "run_params.json"))["blank_key"] is True
    want = {s: statuses.count(s) for s in ("blank", "partly blank", "complete")}
    assert f"blank key: {want['blank']} blank, {want['partly blank']} partly blank, {want['complete']} complete images" in out


def test_cli_key_path_and_other_outputs_together(workdir, plain_run, tmp_path):
    run, _ = _run(workdir, "key_aug", ("--blank-key", str(tmp_path / "k.csv"), "--save-crop", "--half"))
    names, _, recs = _expected(workdir)
    assert open(tmp_path / "k.csv").read() == _key_text(names, recs) and not os.path.exists(run / blank.KEY_FILE)


def test_cli_resume_after_half_of_the_files_gives_the_same_key(workdir):
    import shutil
    names, _, recs = _expected(workdir)
    (workdir / "half").mkdir()
    for n in names[::2]:
        shutil.copy(workdir / "jpegs" / n, workdir / "half" / n)
    run, _ = _run(workdir, "resumed", ("--blank-key",), source="half")
    assert open(run / blank.KEY_FILE).read() == _key_text(names[::2], recs[::2])
    for n in names[1::2]:
        shutil.copy(workdir / "jpegs" / n, workdir / "half" / n)
    refusal = _run(workdir, "resumed", ("--resume",), source="half", ok=False)[1]        # without the flag: refused, as for --save-crop
    assert "blank_key" in refusal
    run, out = _run(workdir, "resumed", ("--blank-key", "--resume"), source="half")
    assert open(run / blank.KEY_FILE).read() == _key_text(names, recs)
    assert f"resume: {len(names[::2])} tiles recorded as done" in out


def test_cli_scene_mode_with_a_white_margin(tmp_path, lib):
    from PIL import Image
    from aquaculture_amd import checkpoint, scenes, tiles
    checkpoint.write_synthetic_checkpoint(str(tmp_path / "multilabel_farms_synth.pt"), "yolov5m", 5)
    scene = np.full((1500, 2048, 3), 255, np.uint8)
    scene[:1024, :1024] = tiles.synthetic_tile(19, 1024)
    scene[:1024, 1024:1800] = tiles.synthetic_tile(3, 1024)[:, :776]
    scene[1024:1300, :1024] = tiles.synthetic_tile(20, 1024)[:276]
    (tmp_path / "scenes").mkdir()
    spath = tmp_path / "scenes" / "ORTHOIMAGERY.ORTHOPHOTOS2015_7.tif"
    Image.fromarray(scene).save(spath)
    grid = scenes.tile_grid(2048, 1500)
    cmd = [sys.executable, os.path.join(ROOT, "yolov5", "detect.py"), "--weights", str(tmp_path / "multilabel_farms_synth.pt"),
           "--source", str(tmp_path / "scenes"), "--tile-scenes", "--save-txt", "--save-conf", "--nosave", "--blank-key",
           "--project", str(tmp_path / "runs"), "--name", "scene", "--batch-size", "4"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    names = [scenes.tile_stem(str(spath), x0, y0) + ".tif" for x0, y0, w, h in grid]
    recs = [blank.stats_numpy(np.ascontiguousarray(scene[y0:y0 + h, x0:x0 + w])) for x0, y0, w, h in grid]
    assert open(tmp_path / "runs" / "scene" / blank.KEY_FILE).read() == _key_text(names, recs)
    assert [blank.status(r_)[0] for r_ in recs] == ["complete", "partly blank", "partly blank", "blank"]
