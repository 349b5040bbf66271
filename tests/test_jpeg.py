"""Split JPEG decode: the host entropy decoder (libaqjpeg.so) + the oracle's pixel half against Pillow's
libjpeg-turbo on the CPU -- which PINS the oracle to the library [UPSTREAM cv2.imread] uses -- and the HIP pixel half against both on the
GPU.  Byte for byte everywhere."""
import io
import os

import numpy as np
import pytest
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _jpeg(img, **kw):
    bio = io.BytesIO()
    Image.fromarray(img).save(bio, format="JPEG", **kw)
    return bio.getvalue()


def _pil(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def _cases():
    from aquaculture_amd import tiles
    rng = np.random.default_rng(5)
    noise = lambda h, w: rng.integers(0, 255, (h, w, 3), dtype=np.uint8)
    smooth = lambda h, w: np.clip(np.add.outer(np.arange(h) * 0.7, np.arange(w) * 0.4)[..., None] + rng.normal(0, 6, (h, w, 3)) + [20, 70, 110], 0, 255).astype(np.uint8)
    return [
        ("ocean tile 640, q75 (the GDAL default of reference tile_tifs.py:74)", _jpeg(tiles.synthetic_tile(3, 640), quality=75)),
        ("cage tile 640", _jpeg(tiles.synthetic_tile(19, 640), quality=75)),
        ("noise 128x192 q90", _jpeg(noise(128, 192), quality=90)),
        ("noise 100x150 q50 (ragged: partial MCUs on both edges)", _jpeg(noise(100, 150), quality=50)),
        ("noise 33x17 q80", _jpeg(noise(33, 17), quality=80)),
        ("smooth 641x1023", _jpeg(smooth(641, 1023), quality=75)),
        ("restart markers every 3 MCUs", _jpeg(noise(64, 64), quality=75, restart_marker_blocks=3)),
        ("restart markers every row", _jpeg(smooth(96, 160), quality=85, restart_marker_rows=1)),
        ("optimised Huffman tables, q95", _jpeg(noise(48, 80), quality=95, optimize=True)),
        ("one MCU, q10", _jpeg(noise(16, 16), quality=10)),
        ("saturated colours (range limit in every stage)", _jpeg(np.tile(np.array([[[255, 0, 0], [0, 255, 0]], [[0, 0, 255], [255, 255, 255]]], np.uint8).repeat(8, 0).repeat(8, 1), (4, 4, 1)), quality=100)),
    ]


@pytest.fixture(scope="module")
def jpeg_lib():
    from aquaculture_amd import build, jpeg
    build.build()
    return jpeg


def test_libaqjpeg_exports_what_its_header_declares(jpeg_lib):
    import re
    hdr = open(os.path.join(ROOT, "include", "aq_jpeg.h")).read()
    names = set(re.findall(r"^int\s+(aq_jpeg_\w+)\s*\(", hdr, re.M))                 # (the device-side entry aq_jpeg_huffman_decode lives in aq_engine.h / libaqengine.so)
    assert names == {"aq_jpeg_decode_coeffs", "aq_jpeg_scan", "aq_jpeg_prepare", "aq_jpeg_prepare_files"}
    lib = jpeg_lib.load_lib()
    for n in names:
        assert hasattr(lib, n), n


@pytest.mark.parametrize("idx", range(11))
def test_entropy_decoder_plus_oracle_equals_pillow(jpeg_lib, idx):
    from oracle import jpeg_oracle as J
    name, data = _cases()[idx]
    ref = _pil(data)
    H, W = ref.shape[:2]
    coef = np.zeros(jpeg_lib.coef_count(H, W), np.int16)
    qt = np.zeros((3, 64), np.uint16)
    rc, info = jpeg_lib.decode_coeffs(data, coef, qt)
    assert rc == 0 and (info.height, info.width) == (H, W), (name, rc)
    got = J.decode_from_coeffs(coef, qt, W, H, info.mcu_cols, info.mcu_rows)
    assert np.array_equal(got, ref), f"{name}: {int((got != ref).sum())} bytes differ"


def test_files_outside_the_split_decoder_are_refused_not_misread(jpeg_lib):
    rng = np.random.default_rng(2)
    img = rng.integers(0, 255, (32, 48, 3), dtype=np.uint8)
    for kw in (dict(subsampling=0), dict(subsampling=1), dict(progressive=True)):
        assert jpeg_lib.scan(_jpeg(img, **kw)) is None, kw
    grey = _jpeg(img[..., 0])
    assert jpeg_lib.scan(grey) is None                                   # one component: the caller's software path
    good = _jpeg(img)
    assert jpeg_lib.scan(good) is not None
    coef = np.zeros(jpeg_lib.coef_count(32, 48), np.int16)
    qt = np.zeros((3, 64), np.uint16)
    for cut in (len(good) // 2, len(good) - 3, 30):                      # truncated files are CORRUPT (next test: exactly where Pillow raises)
        rc, _ = jpeg_lib.decode_coeffs(good[:cut], coef, qt)
        assert rc == -2, rc
    rc, _ = jpeg_lib.decode_coeffs(good, coef[:100], qt)
    assert rc == -3                                                      # too small a buffer is reported, not overrun
    assert jpeg_lib.decode_coeffs(b"not a jpeg at all", coef, qt)[0] == -2


def test_oversubscribed_huffman_table_is_rejected_before_it_is_built(jpeg_lib):
    """a DHT segment whose counts over-subscribe a code length used to index past look[512] on the stack while the table
    was being built (SOI + DHT with counts[0] = 200 and 200 values; reached through aq_jpeg_scan on file-controlled bytes).  The table is
    now refused before anything is written; the sanitizer build of test_entropy_decoder_survives_mutated_files_under_asan runs the same
    bytes plus DHT-count mutations that keep the segment length consistent."""
    import ctypes as C
    lib = jpeg_lib.load_lib()
    for counts in ([200] + [0] * 15, [2, 5] + [0] * 14, [0] * 8 + [255] + [0] * 7, [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 3]):
        n = sum(counts)
        poc = bytes([0xFF, 0xD8, 0xFF, 0xC4]) + (2 + 17 + n).to_bytes(2, "big") + bytes([0x00] + counts) + bytes(i & 255 for i in range(n))
        assert lib.aq_jpeg_scan(poc, len(poc), C.byref(jpeg_lib.JpegInfo())) == -2, counts
    # a FULL but legal table (the all-ones code included at length 16) is still accepted up to the missing frame header
    counts = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
    ok = bytes([0xFF, 0xD8, 0xFF, 0xC4]) + (2 + 17 + 12).to_bytes(2, "big") + bytes([0x00] + counts) + bytes(range(12))
    assert lib.aq_jpeg_scan(ok, len(ok), C.byref(jpeg_lib.JpegInfo())) == -2          # (no SOF / SOS: corrupt for another reason, no crash)


@pytest.mark.parametrize("kw", [dict(quality=75), dict(quality=60, restart_marker_blocks=2), dict(quality=90, optimize=True)])
def test_truncated_or_interrupted_scans_fail_exactly_where_pillow_fails(jpeg_lib, kw):
    """after EOF or an unexpected marker the bit reader supplies zero bits; the decoder used to turn those into
    'valid' grey blocks and return OK, so a half-written tile got (missing) labels and a done-manifest entry.  Every prefix of a file now
    gets the status Pillow gives it: OK only for the complete file, EOI included; a marker in the middle of the entropy-coded data too."""
    rng = np.random.default_rng(7)
    img = np.clip(rng.normal(128, 40, (48, 80, 3)), 0, 255).astype(np.uint8)
    data = _jpeg(img, **kw)
    coef = np.zeros(jpeg_lib.coef_count(48, 80), np.int16)
    qt = np.zeros((3, 64), np.uint16)

    def pil_ok(d):
        try:
            Image.open(io.BytesIO(d)).load()
            return True
        except Exception:
            return False

    cuts = list(range(4, 40)) + list(range(len(data) - 300, len(data) + 1))
    for cut in cuts:
        rc, _ = jpeg_lib.decode_coeffs(data[:cut], coef, qt)
        assert (rc == 0) == pil_ok(data[:cut]), (cut, len(data), rc)
    assert jpeg_lib.decode_coeffs(data, coef, qt)[0] == 0
    sos = data.index(b"\xff\xda")
    mid = sos + (len(data) - sos) // 2
    for marker in (b"\xff\xd9", b"\xff\xc4", b"\xff\xd3" if "restart_marker_blocks" not in kw else b"\xff\xd9"):
        broken = data[:mid] + marker + data[mid + 2:]
        assert jpeg_lib.decode_coeffs(broken, coef, qt)[0] == -2, marker


def test_rgb_signalled_files_go_to_the_software_decoder(jpeg_lib):
    """libjpeg / Pillow do NOT colour-convert three-component files whose Adobe APP14 marker says transform 0, or which
    have no JFIF / Adobe marker and component ids 'R','G','B'.  The device half always converts YCbCr -> RGB, so the header scan must
    hand such files to the software path.  (Pillow writes JFIF + ids 1,2,3; the variants are made by editing those bytes.)"""
    rng = np.random.default_rng(3)
    img = rng.integers(0, 255, (32, 48, 3), dtype=np.uint8)
    good = _jpeg(img, quality=80)
    assert jpeg_lib.scan(good) is not None
    app0 = good.index(b"\xff\xe0")
    app0_len = int.from_bytes(good[app0 + 2:app0 + 4], "big")
    no_jfif = good[:app0] + good[app0 + 2 + app0_len:]
    assert jpeg_lib.scan(no_jfif) is not None                            # no marker, ids 1,2,3: YCbCr by libjpeg's rule
    adobe = lambda t: b"\xff\xee" + (14).to_bytes(2, "big") + b"Adobe" + bytes([0, 100, 0, 0, 0, 0, t])
    assert jpeg_lib.scan(no_jfif[:2] + adobe(0) + no_jfif[2:]) is None   # Adobe transform 0: stored RGB
    assert jpeg_lib.scan(no_jfif[:2] + adobe(1) + no_jfif[2:]) is not None
    assert jpeg_lib.scan(good[:2] + adobe(0) + good[2:]) is not None     # JFIF wins over Adobe (jdapimin.c)
    sof = no_jfif.index(b"\xff\xc0")
    sos = no_jfif.index(b"\xff\xda")
    rgb_ids = bytearray(no_jfif)
    for k, ch in enumerate(b"RGB"):
        rgb_ids[sof + 4 + 6 + 3 * k] = ch
        rgb_ids[sos + 4 + 1 + 2 * k] = ch
    assert jpeg_lib.scan(bytes(rgb_ids)) is None
    ref = np.asarray(Image.open(io.BytesIO(bytes(rgb_ids))).convert("RGB"))
    assert not np.array_equal(ref, _pil(good))                            # and Pillow indeed decodes it differently


@pytest.mark.gpu
def test_device_pixel_half_equals_pillow(jpeg_lib, lib):
    """aq_jpeg_idct_rgb on batches of same-size images: byte-identical to Pillow (and so to the oracle)."""
    import torch
    from aquaculture_amd import engine, tiles
    rng = np.random.default_rng(11)
    groups = {
        (640, 640): [_jpeg(tiles.synthetic_tile(i, 640), quality=75) for i in (0, 3, 19, 40)],
        (1024, 1024): [_jpeg(tiles.synthetic_tile(i, 1024), quality=75) for i in (1, 19)],
        (100, 150): [_jpeg(rng.integers(0, 255, (100, 150, 3), dtype=np.uint8), quality=q) for q in (30, 75, 98)],
        (33, 17): [_jpeg(rng.integers(0, 255, (33, 17, 3), dtype=np.uint8), quality=80)],
        (64, 64): [_jpeg(np.tile(np.array([[[255, 0, 0], [0, 255, 0]], [[0, 0, 255], [255, 255, 255]]], np.uint8).repeat(8, 0).repeat(8, 1), (4, 4, 1)), quality=100)],
    }
    for (H, W), files in groups.items():
        n = jpeg_lib.coef_count(H, W)
        coef = np.zeros((len(files), n), np.int16)
        qt = np.zeros((len(files), 3, 64), np.uint16)
        for i, data in enumerate(files):
            rc, info = jpeg_lib.decode_coeffs(data, coef[i], qt[i])
            assert rc == 0
        off = torch.arange(len(files), dtype=torch.int64) * n
        got = engine.jpeg_idct_rgb(torch.from_numpy(coef).cuda(), off.cuda(), torch.from_numpy(qt.view(np.int16)).cuda(), H, W).cpu().numpy()
        for i, data in enumerate(files):
            ref = _pil(data)
            assert np.array_equal(got[i], ref), f"{H}x{W} image {i}: {int((got[i] != ref).sum())} bytes differ"


def test_entropy_decoder_survives_mutated_files_under_asan(tmp_path):
    """The host decoder parses files it did not write: tests/fuzz_jpeg.c, built with AddressSanitizer + UBSan (CPU build only, as the pool
    asks), decodes thousands of mutated baseline JPEGs into an output buffer of EXACTLY the size the header promises -- flips, truncations,
    damaged tables and lengths, stray markers, runs of 0xFF: every one is either decoded or rejected with a code, none reads or writes out
    of bounds."""
    import shutil
    import subprocess
    from aquaculture_amd import tiles
    cc = shutil.which("gcc")
    if not cc:
        pytest.skip("no gcc")
    rng = np.random.default_rng(1)
    files = []
    for name, img, kw in (("tile.jpg", tiles.synthetic_tile(3, 256), dict(quality=75)),
                          ("noise.jpg", rng.integers(0, 255, (100, 150, 3), dtype=np.uint8), dict(quality=50)),
                          ("restart.jpg", rng.integers(0, 255, (64, 64, 3), dtype=np.uint8), dict(quality=90, restart_marker_blocks=3))):
        (tmp_path / name).write_bytes(_jpeg(img, **kw))
        files.append(str(tmp_path / name))
    exe = str(tmp_path / "fuzz_jpeg")
    r = subprocess.run([cc, "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "fuzz_jpeg.c"),
                        os.path.join(ROOT, "aquaculture_amd", "csrc", "jpeg_coef.c")], capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("this gcc has no sanitizer runtime")
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe, "1500"] + files, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "fuzz_jpeg:" in r.stdout, r.stdout[-500:] + r.stderr[-3000:]
    decoded, rejected = (int(x) for x in __import__("re").findall(r"(\d+) decoded, (\d+) rejected", r.stdout)[0])
    assert decoded > 500 and rejected > 500          # the mutations reach both outcomes


def test_header_scan_in_processes_equals_the_in_process_one(jpeg_lib, tmp_path):
    """Long sweeps scan their files' headers in child processes (jpeg.scan_files_in_processes): same answers as scan_file, file by file --
    sizes for what the split decoder reads, None for a progressive file and for a file that is no JPEG."""
    from aquaculture_amd import tiles
    for i in range(25):
        (tmp_path / f"{i:03d}.jpeg").write_bytes(_jpeg(tiles.synthetic_tile(i, 64 + 16 * (i % 3)), quality=75))
    (tmp_path / "zz_progressive.jpeg").write_bytes(_jpeg(tiles.synthetic_tile(1, 64), quality=75, progressive=True))
    (tmp_path / "zzz_text.jpeg").write_bytes(b"not a jpeg")
    paths = sorted(str(tmp_path / f) for f in os.listdir(tmp_path))
    want = [jpeg_lib.scan_file(p) for p in paths]
    assert want[:3] == [(64, 64), (80, 80), (96, 96)] and want[-2:] == [None, None]
    assert jpeg_lib.scan_files_in_processes(paths, 3) == want
    assert jpeg_lib.scan_files_in_processes(paths[:1], 8) == want[:1]


def _scan_bytes(data):
    """The entropy-coded bytes of a baseline file, from behind the SOS header up to (not including) EOI."""
    sos = data.index(b"\xff\xda")
    start = sos + 2 + int.from_bytes(data[sos + 2:sos + 4], "big")
    end = data.rindex(b"\xff\xd9")
    return data[start:end]


@pytest.mark.parametrize("idx", range(11))
def test_gpu_decode_preparation_is_the_scan_minus_stuffing_and_restart_markers(jpeg_lib, idx):
    """aq_jpeg_prepare (host side of the GPU entropy decode): putting the stuffed zeros and the RSTn markers back into what it wrote gives the
    file's scan bytes exactly; segments are 4-byte aligned, zero-padded, one per restart interval; tables and sizes equal the header scan's."""
    name, data = _cases()[idx]
    ref = _pil(data)
    H, W = ref.shape[:2]
    b = jpeg_lib.GpuDecodeBatch(2, H, W, bytes_per_image=jpeg_lib.stream_capacity(H, W, 12))
    assert b.add(1, data) == 0, name
    sg = b._segs[1]
    rebuilt = bytearray()
    for i, s in enumerate(sg):
        off, ln = int(s["stream_off"]), int(s["stream_len"])
        assert off % 16 == 0 and off >= b.per and not b.streams[off + ln:off + ln + 8].any(), name
        rebuilt += bytes(b.streams[off:off + ln]).replace(b"\xff", b"\xff\x00")
        if i + 1 < len(sg):
            rebuilt += bytes([0xFF, 0xD0 + (i & 7)])
    assert bytes(rebuilt) == _scan_bytes(data), name
    info = jpeg_lib.scan(data)
    assert np.array_equal(b.qt[1], np.ctypeslib.as_array(info.qt).reshape(3, 64))
    total = info.mcu_cols * info.mcu_rows
    assert int(sg["n_mcu"].sum()) == total and int(sg["mcu0"][0]) == 0 and (np.diff(sg["mcu0"].astype(np.int64)) == sg["n_mcu"][:-1]).all()
    assert (sg["coef_off"] == b.nco).all()


def test_gpu_decode_preparation_refuses_what_the_host_decoder_refuses(jpeg_lib):
    rng = np.random.default_rng(2)
    img = rng.integers(0, 255, (32, 48, 3), dtype=np.uint8)
    b = jpeg_lib.GpuDecodeBatch(1, 32, 48, bytes_per_image=jpeg_lib.stream_capacity(32, 48, 12))
    for kw in (dict(subsampling=0), dict(progressive=True)):
        assert b.add(0, _jpeg(img, **kw)) == -1, kw
    assert b.add(0, _jpeg(img[..., 0])) == -1
    good = _jpeg(img, quality=90, restart_marker_blocks=2)
    assert b.add(0, good) == 0
    for cut in (len(good) // 2, len(good) - 2, 40):
        assert b.add(0, good[:cut]) == -2, cut                     # truncated: no EOI
    sos = good.index(b"\xff\xda")
    mid = sos + (len(good) - sos) // 2
    assert b.add(0, good[:mid] + b"\xff\xc4" + good[mid + 2:]) == -2      # a stray marker inside the scan
    rst = good.index(b"\xff\xd0", sos)
    assert b.add(0, good[:rst] + b"\xff\xd3" + good[rst + 2:]) == -2      # restart markers out of sequence
    with pytest.raises(ValueError):
        b.add(0, _jpeg(rng.integers(0, 255, (48, 48, 3), dtype=np.uint8)))  # another size than the batch's


def _bulk_files(tmp_path):
    """21 files of 64 x 64 (16 MCUs): 62 restart segments, 3 table sets (the standard tables and two optimised sets)."""
    rng = np.random.default_rng(21)
    kws = [dict(quality=75)] * 8 + [dict(quality=90, optimize=True)] * 2 + [dict(quality=75, restart_marker_blocks=3)] * 4 + \
          [dict(quality=80, restart_marker_blocks=5)] * 4 + [dict(quality=85, restart_marker_rows=1)] * 3
    order = rng.permutation(len(kws))
    paths, datas = [], []
    for j, k in enumerate(order):
        datas.append(_jpeg(rng.integers(0, 255, (64, 64, 3), dtype=np.uint8), **kws[k]))
        paths.append(str(tmp_path / f"{j:02d}.jpeg"))
        open(paths[-1], "wb").write(datas[-1])
    return paths, datas


@pytest.mark.parametrize("nthreads", [1, 3, 8])
def test_bulk_preparation_equals_add_and_finish(jpeg_lib, tmp_path, nthreads):
    """GpuDecodeBatch.prepare_files -- the C-thread path the sweep uses -- against add + finish on files with and without restart markers
    and with three table sets: the same descriptors field by field, the same table bytes behind every segment's `tabset` (the two paths
    number the sets differently), the same `first`, the same quantisation tables and the same stream bytes over every segment's data
    plus the 8 zero bytes -- in upload buffers that held different stale bytes."""
    paths, datas = _bulk_files(tmp_path)
    H = W = 64
    per = jpeg_lib.stream_capacity(H, W, 12)
    a = jpeg_lib.GpuDecodeBatch(len(paths), H, W, stream_buf=np.full(len(paths) * per + 256, 0xAA, np.uint8), bytes_per_image=per)
    b = jpeg_lib.GpuDecodeBatch(len(paths), H, W, stream_buf=np.full(len(paths) * per + 256, 0x33, np.uint8), bytes_per_image=per)
    for i, d in enumerate(datas):
        assert a.add(i, d) == 0
    segs_a, sets_a, first_a = a.finish()
    segs_b, sets_b, first_b = b.prepare_files(paths, nthreads)
    assert segs_a.shape == segs_b.shape == (62,) and sets_a.shape == sets_b.shape == (3, jpeg_lib.TABSET_BYTES)
    assert (np.diff(first_a) > 1).any() and (np.diff(first_a) == 1).any()
    for f in jpeg_lib.SEG_DTYPE.names:
        if f != "tabset":
            assert np.array_equal(segs_a[f], segs_b[f]), f
    assert np.array_equal(sets_a[segs_a["tabset"]], sets_b[segs_b["tabset"]])
    assert len({bytes(t) for t in sets_b}) == 3
    assert first_a.dtype == first_b.dtype and np.array_equal(first_a, first_b)
    assert np.array_equal(a.qt, b.qt)
    for sg in segs_a:
        o, e = int(sg["stream_off"]), int(sg["stream_off"]) + int(sg["stream_len"]) + 8
        assert np.array_equal(a.streams[o:e], b.streams[o:e]) and not a.streams[e - 8:e].any()


def test_bulk_preparation_names_the_first_offending_file_with_the_reason(jpeg_lib, tmp_path):
    """prepare_files raises ValueError for the FIRST file the GPU decoder does not take, with that file's reason: another size than the
    batch's, no EOI, more restart segments than the bulk path holds per image (73 > SEG_CAP; `add` takes that file), a scan larger than
    bytes_per_image.  A second bad file behind the first is not the one named."""
    rng = np.random.default_rng(22)
    noise = lambda h, w: rng.integers(0, 255, (h, w, 3), dtype=np.uint8)

    def write(name, data):
        (tmp_path / name).write_bytes(data)
        return str(tmp_path / name)

    good = [write(f"good{i}.jpeg", _jpeg(noise(64, 64), quality=75)) for i in range(4)]
    other_size = write("other_size.jpeg", _jpeg(noise(48, 64), quality=75))
    data = _jpeg(noise(64, 64), quality=75)
    no_eoi = write("no_eoi.jpeg", data[:-2])
    per = jpeg_lib.stream_capacity(64, 64, 12)
    for bad, later, why in ((other_size, no_eoi, "not a baseline 8-bit 4:2:0 JPEG of the batch's size"), (no_eoi, other_size, "corrupt or truncated")):
        paths = good[:2] + [bad] + good[2:3] + [later] + good[3:]
        for nthreads in (1, 3):
            with pytest.raises(ValueError) as e:
                jpeg_lib.GpuDecodeBatch(len(paths), 64, 64, bytes_per_image=per).prepare_files(paths, nthreads)
            assert str(e.value).startswith(bad + ":") and why in str(e.value) and later not in str(e.value), str(e.value)
    # 272 x 272 = 17 x 17 MCUs, a restart marker every 4: 73 segments
    many = _jpeg(noise(272, 272), quality=50, restart_marker_blocks=4)
    big = [write(f"big{i}.jpeg", _jpeg(noise(272, 272), quality=50)) for i in range(2)]
    per = jpeg_lib.stream_capacity(272, 272, 12)
    b = jpeg_lib.GpuDecodeBatch(3, 272, 272, bytes_per_image=per)
    assert b.add(1, many) == 0 and b._segs[1].shape[0] == 73 > b.SEG_CAP
    paths = [big[0], write("many_segments.jpeg", many), big[1]]
    with pytest.raises(ValueError) as e:
        b.prepare_files(paths, 2)
    assert str(e.value).startswith(paths[1] + ":") and f"more than {b.SEG_CAP} restart segments" in str(e.value), str(e.value)
    # a scan that does not fit the slot: 0.5 bits per pixel reserved, q = 100 noise takes more than 8
    small = jpeg_lib.stream_capacity(272, 272, 0.5)
    fat = _jpeg(noise(272, 272), quality=100)
    ramp = np.add.outer(np.arange(272), np.arange(272))[..., None].repeat(3, 2) // 3
    lean = [write(f"lean{i}.jpeg", _jpeg((ramp + 20 * i).astype(np.uint8), quality=50)) for i in range(2)]
    assert len(_scan_bytes(fat)) > small
    paths = [lean[0], lean[1], write("fat.jpeg", fat)]
    with pytest.raises(ValueError) as e:
        jpeg_lib.GpuDecodeBatch(3, 272, 272, bytes_per_image=small).prepare_files(paths, 2)
    assert str(e.value).startswith(paths[2] + ":") and "bits per pixel" in str(e.value) and "AQ_JPEG_GPU_BPP" in str(e.value), str(e.value)


@pytest.mark.gpu
def test_gpu_entropy_decode_equals_the_host_decoder(jpeg_lib, lib):
    """aq_jpeg_huffman_decode (one lane per restart segment) on batches of same-size files: the coefficient buffers equal
    aq_jpeg_decode_coeffs's, value for value -- and therefore, through aq_jpeg_idct_rgb, Pillow's pixels byte for byte."""
    import torch
    from aquaculture_amd import engine, tiles
    rng = np.random.default_rng(11)
    noise = lambda h, w: rng.integers(0, 255, (h, w, 3), dtype=np.uint8)
    groups = {
        (640, 640): [_jpeg(tiles.synthetic_tile(i, 640), quality=75) for i in (0, 3, 19, 40)] + [_jpeg(noise(640, 640), quality=q) for q in (50, 95)],
        (1024, 1024): [_jpeg(tiles.synthetic_tile(i, 1024), quality=75) for i in (1, 19)] + [_jpeg(noise(1024, 1024), quality=75, optimize=True)],
        (100, 150): [_jpeg(noise(100, 150), quality=q) for q in (30, 75, 98)] + [_jpeg(noise(100, 150), quality=60, restart_marker_blocks=3)],
        (33, 17): [_jpeg(noise(33, 17), quality=80)],
        (64, 64): [_jpeg(noise(64, 64), quality=75, restart_marker_blocks=3), _jpeg(noise(64, 64), quality=85, restart_marker_rows=1),
                   _jpeg(np.tile(np.array([[[255, 0, 0], [0, 255, 0]], [[0, 0, 255], [255, 255, 255]]], np.uint8).repeat(8, 0).repeat(8, 1), (4, 4, 1)), quality=100)],
    }
    for (H, W), files in groups.items():
        # 70 images: more than one wave of segments, files repeated
        files = (files * 70)[:70]
        n = jpeg_lib.coef_count(H, W)
        want = np.zeros((len(files), n), np.int16)
        qt = np.zeros((len(files), 3, 64), np.uint16)
        for i, data in enumerate(files):
            rc, _ = jpeg_lib.decode_coeffs(data, want[i], qt[i])
            assert rc == 0
        b = jpeg_lib.GpuDecodeBatch(len(files), H, W, bytes_per_image=jpeg_lib.stream_capacity(H, W, 12))
        for i, data in enumerate(files):
            assert b.add(i, data) == 0
        segs, sets, first = b.finish()
        coef = torch.zeros((len(files), n), dtype=torch.int16, device="cuda")
        st = engine.jpeg_huffman_decode(torch.from_numpy(b.streams).cuda(), torch.from_numpy(segs.view(np.uint8).reshape(-1, 32)).cuda(),
                                        torch.from_numpy(sets).cuda(), coef.view(-1))
        assert int(st.abs().max()) == 0, (H, W, st.cpu().tolist())
        got = coef.cpu().numpy()
        assert np.array_equal(b.qt, qt)
        bad = [i for i in range(len(files)) if not np.array_equal(got[i], want[i])]
        assert not bad, f"{H}x{W}: images {bad[:5]} differ ({int((got != want).sum())} values)"
        off = torch.arange(len(files), dtype=torch.int64) * n
        rgb = engine.jpeg_idct_rgb(coef.view(-1), off.cuda(), torch.from_numpy(b.qt.view(np.int16)).cuda(), H, W).cpu().numpy()
        for i in (0, len(files) - 1):
            assert np.array_equal(rgb[i], _pil(files[i]))


def _scan_start(data):
    sos = data.index(b"\xff\xda")
    return sos + 2 + int.from_bytes(data[sos + 2:sos + 4], "big")


def _gpu_decode(streams, segs, sets, n_coef):
    """aq_jpeg_huffman_decode on host arrays: (status [nseg], coefficients [n_coef], canary intact) -- 4096 int16 canaries sit behind the
    coefficient buffer."""
    import torch
    from aquaculture_amd import engine
    coef = torch.zeros(n_coef + 4096, dtype=torch.int16, device="cuda")
    coef[n_coef:] = 12345
    st = engine.jpeg_huffman_decode(torch.from_numpy(streams).cuda(), torch.from_numpy(segs.view(np.uint8).reshape(-1, 32)).cuda(),
                                    torch.from_numpy(sets).cuda(), coef).cpu().numpy()
    out = coef.cpu().numpy()
    return st, out[:n_coef], bool((out[n_coef:] == 12345).all())


@pytest.mark.gpu
def test_gpu_entropy_decode_flags_damaged_scans(jpeg_lib, lib):
    """Bits flipped inside the entropy-coded data (markers intact, so the host preparation accepts the file): every segment either decodes to
    SOME coefficients or reports status 2 -- the kernel terminates, stays inside its buffers (a canary behind them is intact), and a scan cut
    short inside its data (the EOI kept) is reported as consumed-past-the-end.  The same files are refused as by the host decoder, and
    what the host decodes the GPU decodes to the same coefficients -- on standard tables, optimised tables and a file with restart markers
    (there a file counts as decoded only if all its segments are); of the 40 mutated files of every base at least 10 go either way."""
    H, W = 96, 128
    n = jpeg_lib.coef_count(H, W)
    # (seeds picked on the CPU, with the host decoder alone, so that both outcomes are well populated: 21 / 19, 17 / 23 and 20 / 20 of 40)
    for name, seed, kw in (("q80", 5, dict(quality=80)), ("q95 optimised", 13, dict(quality=95, optimize=True)),
                           ("q60 restart rows", 9, dict(quality=60, restart_marker_rows=1))):
        rng = np.random.default_rng(seed)
        good = _jpeg(rng.integers(0, 255, (H, W, 3), dtype=np.uint8), **kw)
        start = _scan_start(good)
        files = [good]
        for k in range(40):
            d = bytearray(good)
            for _ in range(1 + k % 5):
                pos = int(rng.integers(start, len(good) - 2))
                d[pos] = (d[pos] ^ (1 << int(rng.integers(0, 8)))) & 0xFE or 0x01          # never create 0xFF (a marker) by accident
            files.append(bytes(d))
        last = good.rindex(b"\xff\xd4") + 2 if "restart_marker_rows" in kw else start      # (six segments: RST0 .. RST4 between them)
        files.append(good[:last + (len(good) - last) // 3] + b"\xff\xd9")                  # a third of the (last segment's) scan, then EOI
        b = jpeg_lib.GpuDecodeBatch(len(files), H, W, bytes_per_image=jpeg_lib.stream_capacity(H, W, 12))
        keep = [i for i, d in enumerate(files) if b.add(i, d) == 0]
        assert 0 in keep and len(files) - 1 in keep and len(keep) > 30, name
        # compact the accepted files into slots 0.. (finish() wants a prefix)
        b2 = jpeg_lib.GpuDecodeBatch(len(keep), H, W, bytes_per_image=jpeg_lib.stream_capacity(H, W, 12))
        for j, i in enumerate(keep):
            assert b2.add(j, files[i]) == 0
        segs, sets, first = b2.finish()
        st, coef, canary = _gpu_decode(b2.streams, segs, sets, len(keep) * n)
        assert set(st.tolist()) <= {0, 2} and st[0] == 0 and st[-1] == 2, name
        assert canary, name
        host_ok = []
        want, qt = np.zeros((len(keep), n), np.int16), np.zeros((3, 64), np.uint16)
        for j, i in enumerate(keep):
            host_ok.append(jpeg_lib.decode_coeffs(files[i], want[j], qt)[0] == 0)
        gpu_ok = [not st[first[j]:first[j + 1]].any() for j in range(len(keep))]
        assert gpu_ok == host_ok, name                                                  # the same files are refused as by the host decoder
        mutated_ok = sum(host_ok[j] for j, i in enumerate(keep) if 0 < i < len(files) - 1)
        mutated_bad = sum(not host_ok[j] for j, i in enumerate(keep) if 0 < i < len(files) - 1)
        print(f"{name}: {len(keep) - 2} of 40 mutated files prepared, {mutated_ok} decoded by the host, {mutated_bad} refused")
        assert mutated_ok >= 10 and mutated_bad >= 10, (name, mutated_ok, mutated_bad)
        got = coef.reshape(len(keep), n)
        bad = [keep[j] for j in range(len(keep)) if host_ok[j] and not np.array_equal(got[j], want[j])]
        assert not bad, f"{name}: files {bad} decode on both sides, to different coefficients"


# ---- scans that end early: what a lane reads, and how much it does, must not depend on bytes its segment does not own -----------------------
#
# A segment owns [stream_off, stream_off + ((stream_len + 8 + 15) & ~15)) (csrc/jpeg_huff.hip).  The victims below end in EOI but encode fewer
# MCUs than their frame header promises; aq_jpeg_prepare accepts them.  Every stream tensor carries a guard tail of 4 * coef_count + 512
# bytes behind the production-sized n * per + 256: a symbol takes at most 31 bits (16 code + 15 value) and a block at most 64 symbols, so
# even a bit reader without any bound stays inside the allocation, and a kernel that breaks the contract fails by assertion.

_SHORT_SCAN_CASES = ["cut 5 %", "cut 1/3", "cut 99 %", "empty scan 16x16", "restart segment cut", "66 files: tables from global memory",
                     "65 files: tables in LDS"]
_short_scan_cache = {}


def _owned_end(seg):
    return int(seg["stream_off"]) + ((int(seg["stream_len"]) + 8 + 15) & ~15)


def _short_scan_case(jpeg_lib, name):
    """Builds the case's batch (the victim in the LAST slot), decodes it three times -- every non-owned byte behind the victim's owned range
    (the rest of its slot, the spare, the guard; for the restart victim also whatever lies between its segments) filled with zeros, 0x55
    and another image's prepared scan, repeated -- and returns everything the tests look at.  One decode set per case for the module."""
    if name in _short_scan_cache:
        return _short_scan_cache[name]
    rng = np.random.default_rng(5)
    H, W = (16, 16) if "16x16" in name else (96, 128)
    img, img2 = (rng.integers(0, 255, (H, W, 3), dtype=np.uint8) for _ in range(2))
    kw = dict(quality=60, restart_marker_rows=1) if "restart" in name else dict(quality=80)
    good, good2 = _jpeg(img, **kw), _jpeg(img2, quality=80)
    start = _scan_start(good)
    victim_seg = 0                                                     # the cut segment of the victim file
    if name.startswith("cut"):
        frac = {"cut 5 %": 0.05, "cut 1/3": 1 / 3, "cut 99 %": 0.99}[name]
        others, victim = [good, good2], good[:start + int((len(good) - 2 - start) * frac)] + b"\xff\xd9"
    elif "empty" in name:
        others, victim = [good, good2], good[:start] + b"\xff\xd9"     # EOI right behind the SOS header
    elif "restart" in name:
        a, e = good.index(b"\xff\xd0", start) + 2, good.index(b"\xff\xd1", start)
        others, victim, victim_seg = [good2, good], good[:a + (e - a) // 3] + good[e:], 1
    elif "66" in name:
        others = [good, good2] * 32 + [_jpeg(img2, quality=80, optimize=True)]          # lane 0 of the second wave: other tables
        victim = good[:start + (len(good) - start) // 3] + b"\xff\xd9"
    else:
        others, victim = [good, good2] * 32, good[:start + (len(good) - start) // 3] + b"\xff\xd9"
    files = others + [victim]
    nf, n = len(files), jpeg_lib.coef_count(H, W)
    per = jpeg_lib.stream_capacity(H, W, 12)
    b = jpeg_lib.GpuDecodeBatch(nf, H, W, bytes_per_image=per)
    for i, d in enumerate(files):
        assert b.add(i, d) == 0, (name, i)
    segs, sets, first = b.finish()
    assert b.streams.size == nf * per + 256
    vseg = int(first[nf - 1]) + victim_seg
    owned = np.zeros(nf * per + 256 + 4 * n + 512, bool)               # production size + the guard tail
    for sg in segs:
        owned[int(sg["stream_off"]):_owned_end(sg)] = True
    assert owned[:nf * per].any() and not owned[nf * per:].any()
    foreign = ~owned
    foreign[:_owned_end(segs[vseg])] = False                            # non-owned bytes BEHIND the victim's owned range
    donor = b.streams[int(segs[0]["stream_off"]):int(segs[0]["stream_off"]) + int(segs[0]["stream_len"])]
    runs = []
    for fill in ("zeros", "0x55", "scan"):
        streams = np.zeros(owned.size, np.uint8)
        streams[:b.streams.size] = b.streams
        k = int(foreign.sum())
        streams[foreign] = 0 if fill == "zeros" else 0x55 if fill == "0x55" else np.resize(donor, k)
        runs.append(_gpu_decode(streams, segs, sets, nf * n))
    want = np.zeros((nf, n), np.int16)
    host_rc = [jpeg_lib.decode_coeffs(d, want[i], np.zeros((3, 64), np.uint16))[0] for i, d in enumerate(files)]
    intact = np.zeros(n, np.int16)                                      # the victim's file before it was cut
    assert jpeg_lib.decode_coeffs(good, intact, np.zeros((3, 64), np.uint16))[0] == 0
    case = dict(H=H, W=W, n=n, nf=nf, segs=segs, first=first, vseg=vseg, runs=runs, want=want, host_rc=host_rc, intact=intact)
    _short_scan_cache[name] = case
    return case


def _mcu_rows(coef, H, W):
    """[mcu_rows][values]: the coefficients of a 4:2:0 image grouped by MCU row (two Y block rows, one Cb, one Cr)."""
    rows, cols = (H + 15) // 16, (W + 15) // 16
    ny, nc = 4 * rows * cols * 64, rows * cols * 64
    return np.concatenate([coef[:ny].reshape(rows, -1), coef[ny:ny + nc].reshape(rows, -1), coef[ny + nc:].reshape(rows, -1)], axis=1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", _SHORT_SCAN_CASES)
def test_gpu_entropy_decode_of_a_short_scan_ignores_foreign_bytes(jpeg_lib, lib, name):
    """A lane whose segment ends before its MCUs do -- a damaged file, a half-written tile closed properly, a restart interval cut short --
    must not decode what follows its segment.  Whatever the bytes behind the victim's owned range hold, the status vector and the
    coefficient tensor are the same; the victim gets status 2 (the host refuses it too), every other file status 0 and the host decoder's
    coefficients (for the restart victim: every other SEGMENT, the third one's genuine data right behind the cut one), and the canary
    behind the coefficient buffer is intact.  The victim sits in the last slot, so an unbounded reader runs into the spare and the guard.
    Cases: scans cut after 5 %, 1/3 and 99 % of their bytes; an empty scan (stream_len 0); the second of six restart segments cut to a
    third; the victim as lane 1 of a second wave whose lane 0 has other Huffman tables (it reads its own from global memory) and as lane 0
    (tables staged in LDS)."""
    c = _short_scan_case(jpeg_lib, name)
    (st0, coef0, canary0), nf, n, first, vseg = c["runs"][0], c["nf"], c["n"], c["first"], c["vseg"]
    for fill, (st, coef, canary) in zip(("zeros", "0x55", "scan"), c["runs"]):
        assert canary, fill
        assert st.tolist() == st0.tolist(), f"status with {fill} behind the victim's segment differs from the run with zeros"
        diff = int((coef != coef0).sum())
        assert diff == 0, f"{diff} coefficients with {fill} behind the victim's segment differ from the run with zeros"
    assert st0[vseg] == 2 and c["host_rc"][-1] != 0
    assert not np.delete(st0, vseg).any(), st0.tolist()
    assert c["host_rc"][:-1] == [0] * (nf - 1)
    got = coef0.reshape(nf, n)
    bad = [i for i in range(nf - 1) if not np.array_equal(got[i], c["want"][i])]
    assert not bad, f"files {bad} differ from the host decoder's coefficients"
    if vseg != first[nf - 1]:                                           # restart rows: segment s = MCU row s; all but the cut one as in the intact file
        H, W = c["H"], c["W"]
        rows_got, rows_want = _mcu_rows(got[nf - 1], H, W), _mcu_rows(c["intact"], H, W)
        keep = [r for r in range(rows_got.shape[0]) if r != vseg - first[nf - 1]]
        assert len(keep) == 5 and np.array_equal(rows_got[keep], rows_want[keep])


@pytest.mark.gpu
@pytest.mark.parametrize("name", _SHORT_SCAN_CASES)
def test_gpu_entropy_decode_of_a_short_scan_does_bounded_work(jpeg_lib, lib, name):
    """With zeros behind the segment, at most 3 blocks of the victim's buffer are "stray" -- non-zero and different from the intact file's
    block: one block straddles the end of the data; behind the end a lane may use at most 16 more bytes plus the 64 bits already in its
    accumulator, 192 bits in all, and with the standard tables the zero padding costs at least 3 bits per stored coefficient: at most 64
    coefficients, two further blocks.  (A reader without the bound fills every block behind the cut with -1s.  The kernel stops earlier than
    the derivation allows -- no word that ends past stream_len + 8 bytes -- and these cases give 1 or 2 stray blocks; the derivation is not
    tight the other way for every cut, though: zero bits end a chroma block after 4 bits with its DC stored, so a cut inside an MCU's
    fourth Y block can leave that block, Cb, Cr and the next Y block stray.)"""
    c = _short_scan_case(jpeg_lib, name)
    n, nf = c["n"], c["nf"]
    got = c["runs"][0][1].reshape(nf, n)[nf - 1].reshape(-1, 64)
    intact = c["intact"].reshape(-1, 64)
    stray = got.any(axis=1) & (got != intact).any(axis=1)
    print(f"{name}: {int(stray.sum())} stray blocks of {stray.size}")
    assert int(stray.sum()) <= 3, np.nonzero(stray)[0].tolist()
