"""--blank-key on the CPU: the integer statistics (blank.stats_numpy) and the status rule against the literal Pillow / numpy expressions of
the reference's is_blank / is_partly_blank, the fixture recorded from the reference's own functions, and the key file (names, rows, parts,
merge, run_params)."""
import hashlib
import importlib.util
import json
import os

import numpy as np
import pytest
from PIL import Image

from aquaculture_amd import blank

HERE = os.path.dirname(os.path.abspath(__file__))


def literal_status(img):
    """The two reference functions written out: Pillow's extrema of convert("L"), numpy's float averages."""
    im = Image.fromarray(img)
    extrema = im.convert("L").getextrema()
    if extrema == (0, 0) or extrema == (1, 1) or extrema == (255, 255) or (extrema[0] >= 250. and extrema[1] >= 250.):
        return "blank", extrema, None
    rows = np.where(np.average(im, axis=(1, 2)) >= 250.)[0].shape[0]
    cols = np.where(np.average(im, axis=(0, 2)) >= 250.)[0].shape[0]
    return ("partly blank" if rows + cols > 0 else "complete"), extrema, (rows, cols)


def literal_mask_stats(img):
    a = np.asarray(Image.fromarray(img))
    mask = np.all(a < 250, axis=2)
    if not mask.any():
        return 0, (img.shape[1], img.shape[0], -1, -1)
    ys, xs = np.nonzero(mask)
    return int(mask.sum()), (int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max()))


def branch_cases():
    """(name, image): every branch of the two functions, the exact thresholds, the sizes the issue names."""
    rng = np.random.Generator(np.random.PCG64(20261016))
    out = []
    for v in (0, 1, 255, 2):
        out.append((f"all_{v}", np.full((9, 11, 3), v, np.uint8)))
    img = np.full((8, 8, 3), 255, np.uint8); img[3, 4] = 249                       # l_min exactly 249: not blank
    out.append(("lmin_249", img))
    img = np.full((8, 8, 3), 255, np.uint8); img[3, 4] = 250                       # l_min exactly 250: blank
    out.append(("lmin_250", img))
    for w, d in ((16, 1), (16, 0), (1000, 1), (1000, 0)):                          # one row's sum exactly 750 w - 1 / 750 w
        img = rng.integers(0, 100, (12, w, 3)).astype(np.uint8)
        img[5] = 250
        img[5, w // 2, 1] -= d
        out.append((f"row_sum_w{w}_minus{d}", img))
    for h, d in ((16, 1), (16, 0), (1000, 1), (1000, 0)):                          # the same for a column
        img = rng.integers(0, 100, (h, 12, 3)).astype(np.uint8)
        img[:, 7] = 250
        img[h // 3, 7, 2] -= d
        out.append((f"col_sum_h{h}_minus{d}", img))
    img = rng.integers(0, 60, (33, 47, 3)).astype(np.uint8); img[20] = 255
    out.append(("white_row_dark", img))
    img = rng.integers(251, 256, (40, 40, 3)).astype(np.uint8); img[11, 29] = (0, 0, 0)
    out.append(("near_white_one_dark_px", img))
    img = np.full((32, 32, 3), 255, np.uint8); img[..., 0] = rng.integers(0, 256, (32, 32))
    out.append(("one_free_channel", img))
    for h, w in ((1, 1), (7, 13), (640, 640), (1024, 1024), (1000, 1024)):
        out.append((f"random_{h}x{w}", rng.integers(0, 256, (h, w, 3)).astype(np.uint8)))
    img = rng.integers(0, 230, (1024, 1024, 3)).astype(np.uint8); img[:, 900:] = 255; img[1000:] = 254
    out.append(("tile_white_margin", img))
    out.append(("white_1x1", np.full((1, 1, 3), 255, np.uint8)))
    return out


CASES = branch_cases()


@pytest.mark.parametrize("name,img", CASES, ids=[c[0] for c in CASES])
def test_stats_and_status_equal_literal_expressions(name, img):
    s = blank.stats_numpy(img)
    st, extrema, rc = literal_status(img)
    assert (int(s[0]), int(s[1])) == extrema
    assert blank.status(s) == [st]
    if rc is not None:
        assert (int(s[2]), int(s[3])) == rc
    else:                                               # (the reference never looks at rows and columns of a blank image; numpy does here)
        assert int(s[2]) == int((np.average(img, axis=(1, 2)) >= 250.).sum()) and int(s[3]) == int((np.average(img, axis=(0, 2)) >= 250.).sum())
    n, box = literal_mask_stats(img)
    assert int(s[4]) == n and tuple(int(v) for v in s[5:]) == box


def test_every_status_and_threshold_side_is_hit():
    got = {name: blank.status(blank.stats_numpy(img))[0] for name, img in CASES}
    assert set(got.values()) == {"blank", "partly blank", "complete"}
    assert got["all_0"] == got["all_1"] == got["all_255"] == got["lmin_250"] == "blank" and got["all_2"] == "complete"
    assert got["lmin_249"] == "partly blank"            # (its other rows are white)
    for axis in ("row_sum_w16", "row_sum_w1000", "col_sum_h16", "col_sum_h1000"):
        assert got[axis + "_minus1"] == "complete" and got[axis + "_minus0"] == "partly blank", axis
    assert got["near_white_one_dark_px"] == "partly blank" and got["white_row_dark"] == "partly blank"


def test_status_takes_one_record_or_many():
    recs = np.stack([blank.stats_numpy(img) for _, img in CASES[:6]])
    assert blank.status(recs) == [blank.status(r)[0] for r in recs]
    assert recs.dtype == np.int32 and recs.shape[1] == len(blank.FIELDS) == 9


def test_fixture_from_the_reference_functions():
    spec = importlib.util.spec_from_file_location("make_blank_golden", os.path.join(HERE, "golden", "make_blank_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(os.path.join(HERE, "golden", "g10_blank_key.json")) as f:
        cases = json.load(f)["cases"]
    assert {c["status"] for c in cases} == {"blank", "partly blank", "complete"} and any(c["kind"].startswith("jpeg_") for c in cases)
    for c in cases:
        img = gen.build_image(c["kind"], c["h"], c["w"], c["seed"])
        assert img.shape == (c["h"], c["w"], 3)
        assert hashlib.sha256(img.tobytes()).hexdigest() == c["sha256"], c
        assert blank.status(blank.stats_numpy(img)) == [c["status"]], c


def test_name_fields_of_both_tile_name_forms():
    assert blank.name_fields("ORTHOIMAGERY.ORTHOPHOTOS2015_12_1024_2048.jpeg") == ("2015", "12", "1024", "2048")
    assert blank.name_fields("/a/b/ORTHOIMAGERY.ORTHOPHOTOS.ORTHO-EXPRESS.2021_7_0_3072.jpeg") == ("2021", "7", "0", "3072")
    assert blank.name_fields("ORTHOIMAGERY.ORTHOPHOTOS2012_3_0_0.tif") == ("2012", "3", "0", "0")
    for other in ("tile_0001.jpg", "a_b_c_d.jpeg", "ORTHOIMAGERY.ORTHOPHOTOS2015_12_1024.jpeg", "x2015_1_2_3_4.jpeg"):
        assert blank.name_fields(other) == ("", "", "", "")


def _rows(names):
    rng = np.random.Generator(np.random.PCG64(7))
    imgs = [rng.integers(0, 256, (8, 8, 3)).astype(np.uint8) for _ in names]
    imgs[0][:] = 255
    imgs[1][2] = 255
    stats = np.stack([blank.stats_numpy(i) for i in imgs])
    return blank.key_rows(names, stats), stats


def test_key_rows_and_header():
    names = ["/d/ORTHOIMAGERY.ORTHOPHOTOS2015_12_1024_2048.jpeg", "/d/ORTHOIMAGERY.ORTHOPHOTOS.ORTHO-EXPRESS.2021_7_0_3072.jpeg", "/d/odd name.jpg"]
    rows, stats = _rows(names)
    assert blank.HEADER == ",year,bbox_ind,x_offset,y_offset,image_status,image,l_min,l_max,blank_rows,blank_cols,nonblank_px,x0,y0,x1,y1\n"
    assert rows[0] == "2015,12,1024,2048,blank,ORTHOIMAGERY.ORTHOPHOTOS2015_12_1024_2048.jpeg,255,255,8,8,0,8,8,-1,-1"
    assert rows[1].startswith("2021,7,0,3072,partly blank,ORTHOIMAGERY.ORTHOPHOTOS.ORTHO-EXPRESS.2021_7_0_3072.jpeg,")
    assert rows[2].startswith(",,,,complete,odd name.jpg,")
    assert rows[1].split(",")[6:] == [str(int(v)) for v in stats[1]]


def test_merge_of_rank_parts_duplicate_torn_line_and_order(tmp_path):
    names = [f"ORTHOIMAGERY.ORTHOPHOTOS2015_{i}_0_1024.jpeg" for i in range(6)]
    rows, _ = _rows(names)
    d = str(tmp_path)
    p0, p1 = blank.PartFile(d, 0), blank.PartFile(d, 1)
    p0.open(); p1.open()
    p1.append([5, 1], [rows[5], rows[1]])               # ranks and writer threads finish in any order
    p0.append([4, 0], [rows[4], rows[0]])
    p0.append([2], [rows[2]])
    p1.append([3], [rows[3]])
    p0.close(); p1.close()
    with open(blank.part_path(d, 2), "wb") as f:        # an interrupted run of another world size: one tile again, then a line cut short
        f.write(f"1,{rows[1]}\n".encode() + f"3,{rows[3]}"[:-9].encode())
    out = os.path.join(d, blank.KEY_FILE)
    counts = blank.merge_parts(d, out)
    text = open(out).read()
    assert text == blank.HEADER + "".join(f"{i},{rows[i]}\n" for i in range(6))
    assert counts == {"blank": 1, "partly blank": 1, "complete": 4} and not os.path.exists(out + ".tmp")
    # opening a part again drops its torn line; what follows is appended after the last whole one
    p2 = blank.PartFile(d, 2)
    p2.open()
    p2.append([9], ["2015,9,0,0,complete,x.jpeg,1,2,0,0,4,0,0,1,1"], durable=False)
    p2.close()
    assert open(blank.part_path(d, 2)).read() == f"1,{rows[1]}\n9,2015,9,0,0,complete,x.jpeg,1,2,0,0,4,0,0,1,1\n"
    # the consumer: the reference reads the key with pandas and looks at image_status and the four name columns
    pd = pytest.importorskip("pandas")
    df = pd.read_csv(out)
    assert df["image_status"].tolist() == [r.split(",")[4] for r in rows] and df["bbox_ind"].tolist() == list(range(6))
    assert df.columns[0] == "Unnamed: 0" and df.iloc[:, 0].tolist() == list(range(6))


def test_run_params_carry_blank_key_only_when_set():
    from aquaculture_amd.detect import parse_opt, run_params
    base = run_params("w", 0.25, 0.45, 1000, (640, 640), "fp32", True)
    assert "blank_key" not in base
    assert run_params("w", 0.25, 0.45, 1000, (640, 640), "fp32", True, blank_key=True) == {**base, "blank_key": True}
    assert parse_opt(["--source", "x"]).blank_key is None
    assert parse_opt(["--source", "x", "--blank-key"]).blank_key == ""
    assert parse_opt(["--source", "x", "--blank-key", "k.csv"]).blank_key == "k.csv"


def test_resume_refuses_to_mix(tmp_path):
    from aquaculture_amd.detect import run_params
    from aquaculture_amd.manifest import RunParamsMismatch, check_run_params
    check_run_params(str(tmp_path), run_params("w", 0.25, 0.45, 1000, (640, 640), "fp32", True), resume=False)
    with pytest.raises(RunParamsMismatch, match="blank_key"):
        check_run_params(str(tmp_path), run_params("w", 0.25, 0.45, 1000, (640, 640), "fp32", True, blank_key=True), resume=True)
