"""val.py --plots on the GPU: aq_val_mosaic_u8 against val_plots.mosaic_numpy byte for byte (the shapes of tests/test_val_plots.py, views
inside larger allocations, poisoned allocations, CU counts 1, 2, 3 and 13 in child processes), the launcher's refusals, the frame encoder
at quality 75 against Pillow, plot_batch against the Pillow restatement of plot_images, and yolov5/val.py --plots end to end."""
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from poison import poisoned
from test_val_plots import (MOSAIC_CASES, NAMES, case_geometry, case_id, case_images, output_to_target_literal, plot_case, plot_images_literal,
                            stack_targets)

from aquaculture_amd import engine, val, val_plots

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F32 = np.float32
TILES = [0, 1, 2, 3, 19, 20, 21, 22, 23, 24]                                   # the split of tests/test_gpu_val.py
NEW_SYMBOLS = ("aq_val_mosaic_u8", "aq_image_jpeg_coefs_q", "aq_image_jpeg_bytes_q", "aq_write_image_files_q")


def _mosaic(images_dev, geo, **kw):
    xtab, ytab = val_plots.mosaic_tables(geo)
    return engine.val_mosaic(images_dev, geo["n"], geo["ns"], geo["h"], geo["w"], xtab, ytab, **kw)


# ---- bindings ----

def test_the_library_exports_the_new_symbols(lib):
    assert lib.aq_version() == 8
    for name in NEW_SYMBOLS:
        assert name in engine.EXPORTS and hasattr(lib, name), name


# ---- the kernel against the restatement ----

@pytest.mark.parametrize("case", MOSAIC_CASES, ids=case_id)
def test_kernel_equals_mosaic_numpy(lib, case):
    geo = case_geometry(case)
    images = case_images(*case[:3])
    want = val_plots.mosaic_numpy(images, geo)
    got = _mosaic(torch.from_numpy(images).to(DEV), geo)
    assert tuple(got.shape) == want.shape and got.cpu().numpy().tobytes() == want.tobytes()


@pytest.mark.parametrize("offset", (1, 2, 3, 4, 8, 1000))
def test_batches_that_start_inside_a_larger_allocation(lib, offset):
    """The batch is a view `offset` bytes into a larger buffer (any byte alignment), and so is the output (4-byte stores only where the
    address allows): the same bytes, and nothing around the output changes."""
    case = (5, 17, 23, (18, 25))
    geo = case_geometry(case)
    images = case_images(*case[:3])
    want = val_plots.mosaic_numpy(images, geo)
    big = torch.full((offset + images.size + 64,), 0x3C, dtype=torch.uint8, device=DEV)
    big[offset:offset + images.size] = torch.from_numpy(images.reshape(-1)).to(DEV)
    view = big[offset:offset + images.size].view(images.shape)
    obig = torch.full((offset + want.size + 64,), 0x5A, dtype=torch.uint8, device=DEV)
    out = obig[offset:offset + want.size].view(want.shape)
    _mosaic(view, geo, out=out)
    o = obig.cpu().numpy()
    assert o[offset:offset + want.size].tobytes() == want.tobytes()
    assert (o[:offset] == 0x5A).all() and (o[offset + want.size:] == 0x5A).all()


@pytest.mark.parametrize("case", ((5, 17, 23, (18, 25)), (2, 24, 40, (29, 50)), (5, 24, 40, 100), (5, 24, 40, 1920), (10, 24, 40, (25, 41))), ids=case_id)
def test_poisoned_allocations(lib, monkeypatch, case):
    """No byte outside the output changes, and no output byte depends on bytes the kernel does not own: the output's own earlier content,
    and the images of the batch past the first n."""
    geo = case_geometry(case)
    n = geo["n"]
    images = case_images(*case[:3])
    want = val_plots.mosaic_numpy(images, geo)
    for fill in (0xFF, 0x00):
        with poisoned(monkeypatch, fill) as p:
            batch = torch.empty((n + 2, *images.shape[1:]), dtype=torch.uint8, device=DEV)      # two more images, poisoned
            batch[:n].copy_(torch.from_numpy(images))
            got = _mosaic(batch, geo)
            torch.cuda.synchronize()
            p.check_guards()
            assert not p.passed_through and p.intercepted >= 2
            assert got.cpu().numpy().tobytes() == want.tobytes(), hex(fill)


# ---- CU counts ----

VALUES = [None, 1, 2, 3, 13]
_children = {}
_faulted = []


def _child(value, tmp_path_factory):
    if value in _children:
        return _children[value]
    if _faulted:
        pytest.fail(f"not run: an earlier child faulted (AQ_NUM_CUS={_faulted[0]})")
    out = tmp_path_factory.mktemp("plots_cu") / f"cases_{value}.json"
    env = {k: v for k, v in os.environ.items() if k != "AQ_NUM_CUS"}
    if value is not None:
        env["AQ_NUM_CUS"] = str(value)
    r = subprocess.run(["timeout", "-k", "10", "60", sys.executable, os.path.join("tests", "val_plots_cu_cases.py"), "--out", str(out)], cwd=ROOT,
                       env=env, capture_output=True, text=True)
    text = r.stdout[-2000:] + r.stderr[-4000:]
    if r.returncode in (124, 137, 134, 139, -6, -9, -11, 3) or "illegal memory access" in text:
        _faulted.append(value)
    records = {}
    if out.exists():
        data = json.loads(out.read_text())
        assert data["num_cus_env"] == (None if value is None else str(value))
        records = {rec["id"]: rec for rec in data["cases"]}
    _children[value] = (r.returncode, records, text)
    return _children[value]


@pytest.mark.parametrize("value", VALUES, ids=["unset" if v is None else str(v) for v in VALUES])
def test_the_mosaic_does_not_depend_on_the_cu_count(lib, tmp_path_factory, value):
    if _faulted and value not in _children:
        pytest.fail(f"not run: an earlier child faulted (AQ_NUM_CUS={_faulted[0]})")
    if value is not None:
        assert value <= torch.cuda.get_device_properties(0).multi_processor_count
    base_rc, base, base_text = _child(None, tmp_path_factory)
    assert base_rc == 0 and base, f"the unset child exited {base_rc}:\n{base_text}"
    rc, records, text = _child(value, tmp_path_factory)
    assert rc == 0, f"AQ_NUM_CUS={value}: child exited {rc}:\n{text}"
    assert set(records) == set(base) and len(records) == len(MOSAIC_CASES) + 2
    assert all(r["ok"] for r in records.values()), [i for i, r in records.items() if not r["ok"]]
    assert all(r["sha256"] == base[i]["sha256"] for i, r in records.items())
    assert max(r["units"] for r in records.values()) > 32 * 13                  # more units than workgroups at 13 CUs: a second trip


# ---- refusals ----

def test_the_launcher_refuses_by_its_arguments_and_writes_nothing(lib):
    geo = case_geometry((5, 17, 23, (18, 25)))
    n, ns, H, W, h, w = geo["n"], geo["ns"], 17, 23, geo["h"], geo["w"]
    oh, ow = geo["size"]
    images = torch.from_numpy(case_images(5, 17, 23)).to(DEV)
    xtab, ytab = val_plots.mosaic_tables(geo)
    tab = torch.from_numpy(np.concatenate([xtab, ytab])).to(DEV)
    out = torch.full((oh * ow * 3,), 0x5A, dtype=torch.uint8, device=DEV)
    good = dict(batch=images.data_ptr(), batch_bytes=images.numel(), n=n, ns=ns, H=H, W=W, h=h, w=w, out=out.data_ptr(), out_bytes=out.numel(),
                out_h=oh, out_w=ow, xd=tab.data_ptr(), xh=xtab.ctypes.data, yd=tab.data_ptr() + 16 * ow, yh=ytab.ctypes.data)

    def call(**kw):
        a = dict(good, **kw)
        return lib.aq_val_mosaic_u8(a["batch"], a["batch_bytes"], a["n"], a["ns"], a["H"], a["W"], a["h"], a["w"], a["out"], a["out_bytes"],
                                    a["out_h"], a["out_w"], a["xd"], a["xh"], a["yd"], a["yh"], None)

    bad_x, bad_y = xtab.copy(), ytab.copy()
    bad_x[7, 1] = ns * W                                                        # one past the source mosaic
    bad_y[3, 0] = -1
    refusals = [("null", dict(batch=None)), ("null", dict(out=None)), ("null", dict(xd=None)), ("null", dict(xh=None)), ("null", dict(yd=None)),
                ("null", dict(yh=None)), ("images", dict(n=0)), ("images", dict(n=17, ns=5)), ("does not hold", dict(ns=2)),
                ("too large", dict(n=16, ns=5, batch_bytes=1 << 30)), ("bad sizes", dict(H=0)), ("bad sizes", dict(W=-1)), ("bad sizes", dict(h=0)),
                ("bad sizes", dict(w=0)), ("bad sizes", dict(out_h=0)), ("the output is", dict(out_h=oh + 1)), ("the output is", dict(out_w=ow - 1)),
                ("the output is", dict(h=h + 1)), ("the batch holds", dict(batch_bytes=n * H * W * 3 - 1)), ("the batch holds", dict(H=H + 1)),
                ("the output holds", dict(out_bytes=oh * ow * 3 - 1)), ("reads columns", dict(xh=bad_x.ctypes.data)),
                ("reads rows", dict(yh=bad_y.ctypes.data)), ("reads columns", dict(W=W - 1, batch_bytes=1 << 20)),
                ("unaligned", dict(xd=tab.data_ptr() + 4))]
    for word, kw in refusals:
        assert call(**kw) != 0, kw
        assert word in lib.aq_last_error().decode(), (kw, lib.aq_last_error())
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all())
    assert call() == 0                                                          # and the arguments they were varied from are accepted
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == val_plots.mosaic_numpy(images.cpu().numpy(), geo).tobytes()


# ---- the frame encoder's quality ----

def _frames(sizes, seed=3):
    rng = np.random.default_rng(seed)
    out = []
    for w, h in sizes:
        yy, xx = np.mgrid[0:h, 0:w]
        im = np.stack([(xx * 5 + yy * 3) % 256, (xx * 2 + yy * 7) % 256, (xx + yy) * 255 // (w + h)], 2).astype(np.uint8)
        im[h // 4:h // 2, w // 4:w // 2] = rng.integers(0, 256, (h // 2 - h // 4, w // 2 - w // 4, 3), dtype=np.uint8)
        out.append(im)
    return out


def _encode(images, quality):
    nbytes = [(im.size + 3) // 4 * 4 for im in images]
    bases = np.concatenate([[0], np.cumsum(nbytes)[:-1]]).astype(np.int64)
    buf = np.zeros(int(sum(nbytes)), np.uint8)
    for b, im in zip(bases, images):
        buf[b:b + im.size] = im.reshape(-1)
    table = engine.frame_table(bases, [3 * im.shape[1] for im in images], [im.shape[:2] for im in images])
    coef, table = engine.encode_frames(torch.from_numpy(buf).to(DEV), table, quality=quality)
    return coef, table


def _pillow(im, **kw):
    b = io.BytesIO()
    Image.fromarray(im).save(b, format="JPEG", **kw)
    return b.getvalue()


def test_quality_75_frames_are_pillows_bytes(lib, tmp_path):
    images = _frames(((48, 32), (50, 34), (1920, 32)))
    coef, table = _encode(images, 75)
    for i, im in enumerate(images):
        h, w = im.shape[:2]
        got = engine.image_jpeg_bytes(coef[int(table["mcu"][i]):], w, h, quality=75)
        assert got == _pillow(im, quality=75), (w, h)
        assert got == _pillow(im)                                               # Image.save()'s defaults
    names = [f"f{i}.jpg" for i in range(3)]
    assert engine.write_image_files(str(tmp_path), names, coef, table, threads=2, quality=75) == 3
    for name, im in zip(names, images):
        assert (tmp_path / name).read_bytes() == _pillow(im)


def test_quality_95_is_the_existing_entry_point(lib, tmp_path):
    images = _frames(((48, 32), (50, 34), (1920, 32)))
    coef, table = _encode(images, None)
    coef_q, _ = _encode(images, 95)
    assert coef.tobytes() == coef_q.tobytes()
    for i, im in enumerate(images):
        h, w = im.shape[:2]
        old = engine.image_jpeg_bytes(coef[int(table["mcu"][i]):], w, h)
        assert old == engine.image_jpeg_bytes(coef[int(table["mcu"][i]):], w, h, quality=95) == _pillow(im, quality=95, subsampling=2)
    engine.write_image_files(str(tmp_path), ["a/x.jpg"], coef, table[:1], quality=None)
    engine.write_image_files(str(tmp_path), ["b/x.jpg"], coef, table[:1], quality=95)
    assert (tmp_path / "a" / "x.jpg").read_bytes() == (tmp_path / "b" / "x.jpg").read_bytes() == _pillow(images[0], quality=95, subsampling=2)


def test_the_encoder_refuses_other_qualities(lib):
    images = _frames(((48, 32),))
    for q in (0, 101, -5):
        with pytest.raises(RuntimeError, match="quality"):
            _encode(images, q)
    coef, table = _encode(images, 50)
    assert lib.aq_image_jpeg_bytes_q(coef.ctypes.data, 48, 32, 0, None, 0) == 0
    assert engine.image_jpeg_bytes(coef, 48, 32, quality=50) == _pillow(images[0], quality=50)
    assert engine.image_jpeg_bytes(*_encode(images, 1)[:1], 48, 32, quality=1) == _pillow(images[0], quality=1)
    assert engine.image_jpeg_bytes(*_encode(images, 100)[:1], 48, 32, quality=100) == _pillow(images[0], quality=100)


# ---- plot_batch ----

@pytest.mark.parametrize("max_size", (60, 1920), ids=("resize", "paste"))
def test_plot_batch_writes_what_pillow_saves(lib, tmp_path, max_size):
    n, H, W, h0, w0 = 5, 24, 40, 48, 80
    images = case_images(n, H, W)
    labels, dets, counts, paths = plot_case(n, H, W, h0, w0, seed=11)
    max_det = max(counts)
    det_all = np.full((n, max_det, 6), np.nan, F32)
    for i, d in enumerate(dets):
        det_all[i, :counts[i]] = d
    ltg, ptg = val_plots.batch_targets(det_all, np.asarray(counts), labels, (h0, w0), (H, W))
    geo = val_plots.plot_batch(torch.from_numpy(images).to(DEV), paths, ltg, ptg, NAMES, str(tmp_path), ("val_batch0_labels.jpg", "val_batch0_pred.jpg"),
                               max_size=max_size)
    assert geo["resized"] == (max_size == 60)
    mosaic = val_plots.mosaic_numpy(images, geo)
    for name, targets in (("labels", stack_targets(ltg)), ("pred", output_to_target_literal(dets))):
        want_px = plot_images_literal(mosaic.copy(), n, H, W, targets, paths, str(tmp_path / f"want_{name}.jpg"), NAMES, max_size)
        got = (tmp_path / f"val_batch0_{name}.jpg").read_bytes()
        assert got == (tmp_path / f"want_{name}.jpg").read_bytes(), name
        assert np.asarray(Image.open(io.BytesIO(got))).shape == want_px.shape
        assert (want_px != mosaic).any()


# ---- the command line ----

@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    """The synthetic checkpoint and ten synthetic 640-px jpegs, labelled by yolov5/detect.py's own fp32 detections, as tests/test_gpu_val.py
    builds its split: images/, labels/ and a data.yaml."""
    from aquaculture_amd import checkpoint, tiles
    d = tmp_path_factory.mktemp("val_plots")
    tiles.write_synthetic_jpegs(str(d / "set" / "images"), TILES, size=640)
    checkpoint.write_synthetic_checkpoint(str(d / "multilabel_farms_synth.pt"), "yolov5m", 5)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "yolov5", "detect.py"), "--weights", str(d / "multilabel_farms_synth.pt"), "--source",
                        str(d / "set" / "images"), "--nosave", "--save-txt", "--save-conf", "--project", str(d / "runs"), "--name", "detect",
                        "--batch-size", "4"], capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    os.makedirs(d / "set" / "labels")
    for f in sorted(os.listdir(d / "runs" / "detect" / "labels")):
        lines = [" ".join(l.split()[:5]) for l in open(d / "runs" / "detect" / "labels" / f).read().splitlines()]
        (d / "set" / "labels" / f).write_text("\n".join(dict.fromkeys(lines)) + "\n")
    ck = checkpoint.load_checkpoint(str(d / "multilabel_farms_synth.pt"))
    (d / "data.yaml").write_text(f"path: {d / 'set'}\nval: images\nnames:\n" + "".join(f"  {i}: {ck.names[i]}\n" for i in range(5)))
    return d


def _val(d, name, *extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "yolov5", "val.py"), "--data", str(d / "data.yaml"), "--weights",
                        str(d / "multilabel_farms_synth.pt"), "--save-txt", "--save-conf", "--confusion-matrix", "--project", str(d / "runs"),
                        "--name", name, "--batch-size", "4", *extra], capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    head = lines.index(val.TABLE_HEADER)
    return d / "runs" / name, [l for l in lines[head:] if not l.startswith(("Speed:", "Results saved", "val:")) and "saved to" not in l]


def _tree(run):
    return {os.path.relpath(os.path.join(b, f), run): open(os.path.join(b, f), "rb").read() for b, _, fs in os.walk(run) for f in fs}


def test_val_plots_end_to_end_and_nothing_else_changes(dataset, lib):
    d = dataset
    plain, table0 = _val(d, "plain")
    run, table1 = _val(d, "plots", "--plots")
    assert table0 == table1
    a, b = _tree(plain), _tree(run)
    mosaics = {f"val_batch{i}_{k}.jpg" for i in range(3) for k in ("labels", "pred")}
    assert set(b) - set(a) == mosaics and set(a) <= set(b) and len(a) > 10 + 5
    for f in a:
        if f != "val.json":
            assert a[f] == b[f], f
    ja, jb = json.loads(a["val.json"]), json.loads(b["val.json"])
    plots = jb.pop("plots")
    for j in (ja, jb):
        j.pop("images_per_s")                                                   # the one timing in val.json
    assert "plots" not in ja and ja == jb
    assert [p["labels"] for p in plots["batches"]] == [f"val_batch{i}_labels.jpg" for i in range(3)]
    assert [p["images"] for p in plots["batches"]] == [4, 4, 2]
    for p in plots["batches"]:
        geo = val_plots.mosaic_geometry(p["images"], 640, 640)
        assert (p["height"], p["width"]) == geo["size"]
        for k in ("labels", "pred"):
            im = Image.open(io.BytesIO(b[p[k]]))
            im.load()
            assert im.size == (p["width"], p["height"]) and im.mode == "RGB"
            px = np.asarray(im)
            assert px.std() > 10                                                # a picture, not a blank canvas
    assert b["val_batch0_labels.jpg"] != b["val_batch0_pred.jpg"]
