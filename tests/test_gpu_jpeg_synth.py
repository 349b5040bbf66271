"""The device half of the JPEG decode (aq_jpeg_idct_rgb_checked) and the GPU Huffman kernel on files built from chosen coefficients
(tests/jpeg_synth.py): pixels against Pillow's libjpeg-turbo decode of the file itself right up to the acceptance rule, the rule's flag on
the device against oracle/jpeg_oracle.accepted, coefficient buffers against the coefficients that went into the file, and detect.py's
refusal of a file outside the rule.  The CPU side of the same files is tests/test_jpeg_synth.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import jpeg_synth as S
from oracle import jpeg_oracle as J

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def jpeg_lib():
    from aquaculture_amd import build, jpeg
    build.build()
    return jpeg


def _device_decode(jpeg_lib, files, h, w, lead=192):
    """The files (one size) through the host entropy decoder and ONE aq_jpeg_idct_rgb_checked launch, every image with its own tables, the
    first image `lead` int16 into the coefficient buffer.  -> (rgb uint8 [n, h, w, 3], flags [n], canaries intact, coef [n, count], qt)."""
    import torch
    from aquaculture_amd import engine
    n, cnt = len(files), jpeg_lib.coef_count(h, w)
    coef = np.zeros((n, cnt), np.int16)
    qt = np.zeros((n, 3, 64), np.uint16)
    for i, data in enumerate(files):
        coef[i], qt[i], _ = S.host_decode(jpeg_lib, data, h, w)
    buf = np.full(lead + n * cnt, 31000, np.int16)                      # (the lead holds values that would be refused if they were read)
    buf[lead:] = coef.reshape(-1)
    off = torch.arange(n, dtype=torch.int64) * cnt + lead
    nb = n * h * w * 3
    out = torch.full((nb + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    flags = torch.full((n + 64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    rgb, fl = engine.jpeg_idct_rgb_checked(torch.from_numpy(buf).cuda(), off.cuda(), torch.from_numpy(qt.view(np.int16)).cuda(), h, w,
                                           out=out[:nb].view(n, h, w, 3), flags=flags)
    torch.cuda.synchronize()
    intact = bool((out[nb:] == 0xA5).all()) and bool((flags[n:] == 0x5A5A5A5A).all())
    return rgb.cpu().numpy(), fl.cpu().numpy(), intact, coef, qt


@pytest.mark.parametrize("size", S.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_pixel_half_equals_pillow_up_to_the_limit(jpeg_lib, lib, size):
    """Eight images of one size in one launch, each with its own tables (all ones, random 1..255, all 255, 16-bit random 1..1000: twice
    each) and its own pattern, blocks pushed up to WS_MAX, the first image 192 values into the coefficient buffer: every byte equals
    Pillow's decode of the file, every flag is 0, nothing is written behind the output or the flags."""
    h, w = size
    rows, cols = S.mcus(h, w)
    files = []
    for i in range(8):
        rng = np.random.default_rng([h, w, i])
        tables, pq = S.make_tables(S.TABLE_KINDS[i % 4], rng)
        coef = S.gen_blocks(rng, rows * cols, tables, S.PATTERNS[(i + i // 4) % 4], J.WS_MAX)
        files.append(S.file_from_coeffs(coef, w, h, tables, pq))
    rgb, flags, intact, coef, qt = _device_decode(jpeg_lib, files, h, w)
    top = max(S.file_ws_max(coef[i], qt[i], cols, rows) for i in range(8))
    print(f"{h}x{w}: largest |ws| {top}")
    assert J.WS_MAX - 64 <= top <= J.WS_MAX
    assert intact
    assert not flags.any(), flags.tolist()
    for i, data in enumerate(files):
        ref = S.pil_rgb(data)
        assert np.array_equal(rgb[i], ref), f"image {i}: {int((rgb[i] != ref).sum())} of {ref.size} bytes differ"


def test_device_pixel_half_on_every_basis_function(jpeg_lib, lib):
    """Each of the 64 coefficients alone at +1023 and at -1023 with a table of 4 (|coef q| = 4092), in all six blocks of a 16 x 16 image --
    Y, Cb and Cr: 128 images in one launch.  Range limiting in both directions and the colour clamp in every channel.  A lone DC or c4
    gives |ws| = 16368, inside the rule; the other rows' gains are up to 1.39 times that (|ws| up to 22.7 k), so most of these images are
    REFUSED: the flags equal accepted(), and the pixels equal Pillow's all the same -- a single basis function at this amplitude is still
    within what the library's 16-bit workspace holds, the rule refuses it because sums of two such values are not."""
    t4 = (np.full(64, 4), np.full(64, 4))
    files = []
    for k in range(64):
        for sgn in (1, -1):
            c = np.zeros((1, 6, 64), np.int64)
            c[0, :, k] = sgn * 1023
            files.append(S.file_from_coeffs(c, 16, 16, t4))
    rgb, flags, intact, coef, qt = _device_decode(jpeg_lib, files, 16, 16)
    ok = [S.file_accepted(coef[i], qt[i], 1, 1) for i in range(128)]
    assert intact and 0 < sum(ok) < 128
    assert flags.tolist() == [0 if a else 1 for a in ok]
    ref = np.stack([S.pil_rgb(d) for d in files])
    assert ref.min() == 0 and ref.max() == 255
    bad = [i for i in range(128) if not np.array_equal(rgb[i], ref[i])]
    assert not bad, f"coefficient / sign {[(i // 2, '+-'[i % 2]) for i in bad[:8]]}: {int((rgb != ref).sum())} bytes differ"


def test_the_rule_on_the_device(jpeg_lib, lib):
    """One batch of 29 images of 17 x 16 (2 MCUs, 12 blocks) that interleaves accepted and refused ones, five blocks that alias behind them.  Every image is full of blocks up
    to WS_MAX; image i then gets ONE block found by search -- max |ws| in [WS_MAX - 7, WS_MAX] for even i, in [WS_MAX + 1, WS_MAX + 8] for odd
    i -- at a block position that moves through Y, Cb and Cr of both MCUs; the last two refused images are far outside instead (a flat
    DC of 1000 x 16, and one block of dense +-1023 x 255 whose 32-bit arithmetic wraps).  The flags equal accepted() image by image, the
    accepted images equal Pillow, and nothing is written behind the output or the flags."""
    h, w, n = 17, 16, 24
    rows, cols = S.mcus(h, w)
    files, want = [], []
    for i in range(n):
        rng = np.random.default_rng([77, i])
        tables = (rng.integers(1, 9, 64), rng.integers(1, 9, 64))
        coef = S.gen_blocks(rng, rows * cols, tables, S.PATTERNS[i % 4], J.WS_MAX)
        mcu, blk = (i // 2) % 2, (i * 5 + i // 12) % 6
        lo, hi = (J.WS_MAX + 1, J.WS_MAX + 8) if i % 2 else (J.WS_MAX - 7, J.WS_MAX)
        if i == n - 1:
            tables = (np.full(64, 255), np.full(64, 255))
            coef[:] = 0
            coef[mcu, blk] = rng.choice([-1023, 1023], 64)
        elif i == n - 3:
            tables = (np.full(64, 16), np.full(64, 16))
            coef[:] = 0
            coef[:, :, 0] = 1000
        else:
            coef[mcu, blk] = S.block_in_window(rng, tables[0 if blk < 4 else 1], lo, hi, S.PATTERNS[(i // 2) % 4])
        files.append(S.file_from_coeffs(coef, w, h, tables))
        want.append(i % 2 == 0)
    # blocks whose 32-bit pass 1 WRAPS BACK inside the limit (|ws| in the millions; wrapped: 9212, 16352, 0, 0 and under 16384): a kernel that
    # judged its own wrapped workspace would pass them.  One coefficient each, (index, value, table entry): DC 2047 x 255 and 2040 x 255
    # with 8-bit tables; DC 512 x 1024, c4 (index 32) 512 x 1024 and the AC value 994 x 28259 at index 16 with 16-bit tables.
    for j, (k, c, q) in enumerate(((0, 2047, 255), (0, 2040, 255), (0, 512, 1024), (32, -512, 1024), (16, 994, 28259))):
        tab = np.ones(64, np.int64)
        tab[k] = q
        coef = np.zeros((rows * cols, 6, 64), np.int64)
        coef[j % 2, (0, 4, 5, 3, 2)[j], k] = c
        files.append(S.file_from_coeffs(coef, w, h, (tab, tab), int(q > 255)))
        want.append(False)
    rgb, flags, intact, coef, qt = _device_decode(jpeg_lib, files, h, w)
    ok = [S.file_accepted(coef[i], qt[i], cols, rows) for i in range(len(files))]
    tops = [S.file_ws_max(coef[i], qt[i], cols, rows) for i in range(len(files))]
    print("max |ws| per image:", tops)
    assert ok == want and min(tops[n:]) > 100 * J.WS_MAX
    assert all(J.WS_MAX - 7 <= t <= J.WS_MAX for t in tops[0:n:2]) and all(J.WS_MAX < t <= J.WS_MAX + 8 for t in tops[1:n - 3:2])
    assert intact
    assert flags.tolist() == [0 if a else 1 for a in ok]
    for i in range(0, n, 2):
        ref = S.pil_rgb(files[i])
        assert np.array_equal(rgb[i], ref), f"accepted image {i}: {int((rgb[i] != ref).sum())} bytes differ"


def test_unchecked_entry_gives_the_same_pixels(jpeg_lib, lib):
    """aq_jpeg_idct_rgb (kept for callers built against it; engine.jpeg_idct_rgb goes through the checked entry) is the checked entry with
    no flags: called as the C library exports it."""
    import torch
    from aquaculture_amd import engine
    h, w = 31, 33
    rows, cols = S.mcus(h, w)
    rng = np.random.default_rng(4)
    tables, pq = S.make_tables("random", rng)
    data = S.file_from_coeffs(S.gen_blocks(rng, rows * cols, tables, "dense", J.WS_MAX), w, h, tables, pq)
    coef, qt, _ = S.host_decode(jpeg_lib, data, h, w)
    coef_d, qt_d = torch.from_numpy(coef).cuda(), torch.from_numpy(qt.view(np.int16)).cuda()
    off_d = torch.zeros(1, dtype=torch.int64, device="cuda")
    scratch = torch.empty(lib.aq_jpeg_scratch_bytes(1, h, w), dtype=torch.uint8, device="cuda")
    out = torch.zeros((1, h, w, 3), dtype=torch.uint8, device="cuda")
    assert lib.aq_jpeg_idct_rgb(coef_d.data_ptr(), off_d.data_ptr(), qt_d.data_ptr(), 1, h, w, scratch.data_ptr(), out.data_ptr(), engine._stream_ptr()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy()[0], S.pil_rgb(data))
    assert np.array_equal(engine.jpeg_idct_rgb(coef_d, off_d, qt_d, h, w).cpu().numpy()[0], S.pil_rgb(data))


@pytest.mark.parametrize("size", [(16, 16), (33, 17), (64, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_gpu_entropy_decode_returns_the_coefficients_that_went_in(jpeg_lib, lib, size):
    """aq_jpeg_huffman_decode through GpuDecodeBatch on 70 files (more than one wave of lanes) written from chosen coefficients: +-1023 in
    all 64 positions with the DC alternating (differences of 2046), a DC ramp in steps of 2047, only index 63 non-zero, empty blocks, long
    zero runs, dense random values.  Status all zero; the buffers equal expected_layout of what went in -- the truth, independent of both
    decoders -- and aq_jpeg_decode_coeffs's output, value for value."""
    import torch
    from aquaculture_amd import engine
    h, w = size
    rows, cols = S.mcus(h, w)
    ones = (np.ones(64, np.int64), np.ones(64, np.int64))
    cases = [(name, c) for name, hw, c in S.extreme_coefficient_files() if hw == (h, w)]
    assert len(cases) == 5
    files = [S.file_from_coeffs(c, w, h, ones) for _, c in cases]
    truth = [S.expected_layout(c, cols, rows) for _, c in cases]
    order = [(i * 3 + i // 5) % 5 for i in range(70)]
    n = jpeg_lib.coef_count(h, w)
    b = jpeg_lib.GpuDecodeBatch(70, h, w, bytes_per_image=jpeg_lib.stream_capacity(h, w, 48))
    for i, k in enumerate(order):
        assert b.add(i, files[k]) == 0, cases[k][0]
    segs, sets, first = b.finish()
    coef = torch.zeros(70 * n + 4096, dtype=torch.int16, device="cuda")
    coef[70 * n:] = 12345
    st = engine.jpeg_huffman_decode(torch.from_numpy(b.streams).cuda(), torch.from_numpy(segs.view(np.uint8).reshape(-1, 32)).cuda(),
                                    torch.from_numpy(sets).cuda(), coef)
    assert int(st.abs().max()) == 0, st.cpu().tolist()
    got = coef.cpu().numpy()
    assert (got[70 * n:] == 12345).all()
    got = got[:70 * n].reshape(70, n)
    for k, (name, _) in enumerate(cases):
        host, _, _ = S.host_decode(jpeg_lib, files[k], h, w)
        assert np.array_equal(host, truth[k]), name
    bad = [(i, cases[k][0]) for i, k in enumerate(order) if not np.array_equal(got[i], truth[k])]
    assert not bad, bad[:5]


def test_cli_refuses_a_file_outside_the_rule_in_both_gpu_routes(jpeg_lib, lib, tmp_path):
    """One refused file (a flat image of DC 1000 with a table of 16) among 40 accepted 64 x 64 files: --jpeg-decode split and --jpeg-decode gpu
    end with an error that names that file, the rule and --jpeg-decode host, and neither a label file nor a manifest entry exists for any
    file of its batch of 4; --jpeg-decode host completes."""
    from aquaculture_amd import checkpoint
    src = tmp_path / "jpegs"
    src.mkdir()
    rows, cols = S.mcus(64, 64)
    names = [f"t{i:02d}" for i in range(41)]
    victim = names[22]
    for i, nm in enumerate(names):
        rng = np.random.default_rng([9, i])
        if nm == victim:
            tables = (np.full(64, 16), np.full(64, 16))
            coef = np.zeros((rows * cols, 6, 64), np.int64)
            coef[:, :, 0] = 1000
        else:
            tables, _ = S.make_tables("random", rng)
            coef = S.gen_blocks(rng, rows * cols, tables, "sparse", J.WS_MAX // 2)
        (src / (nm + ".jpeg")).write_bytes(S.file_from_coeffs(coef, 64, 64, tables))
    weights = tmp_path / "multilabel_farms_synth.pt"
    checkpoint.write_synthetic_checkpoint(str(weights), "yolov5m", 5)
    batch = names[20:24]
    for mode in ("host", "split", "gpu"):
        cmd = [sys.executable, os.path.join(ROOT, "yolov5", "detect.py"), "--weights", str(weights), "--source", str(src), "--nosave", "--save-txt",
               "--save-conf", "--project", str(tmp_path / "runs"), "--name", "rule_" + mode, "--batch-size", "4", "--half", "--quiet",
               "--conf-thres", "0.001", "--jpeg-decode", mode]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=420, env=dict(os.environ, AQ_JPEG_GPU_BPP="24"))
        run = tmp_path / "runs" / ("rule_" + mode)
        done = set(open(run / "done.rank0.txt").read().split()) if (run / "done.rank0.txt").exists() else set()
        labels = {os.path.splitext(f)[0] for f in os.listdir(run / "labels")} if (run / "labels").exists() else set()
        if mode == "host":                                         # the checkpoint does label these files: the absences below mean something
            assert r.returncode == 0, r.stderr[-2000:]
            assert set(names) <= done
            assert len(labels) >= 30 and names[0] in labels and (set(batch) - {victim}) & labels, sorted(labels)
            continue
        assert r.returncode != 0, (mode, r.stdout[-1500:])
        err = r.stderr[-3000:]
        assert "ValueError" in err and victim + ".jpeg" in err and "acceptance rule" in err and "--jpeg-decode host" in err, (mode, err)
        assert not [nm for nm in names if nm != victim and nm + ".jpeg" in err], (mode, err)
        assert not (set(batch) & done) and not (set(batch) & labels), (mode, sorted(done), sorted(labels))
        assert names[0] in done and names[0] in labels, (mode, sorted(done), sorted(labels))     # earlier batches were written and recorded
