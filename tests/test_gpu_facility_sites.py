"""--facility-sites on the GPU: aq_facility_bounds_f64, aq_box_join_count_i32 and aq_box_join_list_i32 (csrc/facility_sites.hip) through
engine.facility_bounds / box_join_count / box_join_list against the numpy restatements (facility_sites.bounds_numpy, join_count_numpy,
join_list_numpy), bit for bit (``tobytes()``), every output allocated poisoned and between guard regions; the lane-stride edges of the
three kernels and the edges of the ballot prefix; the fixture of tests/test_facility_sites.py end to end; the launchers' refusals; one
detect.py run in a child process under its own time limit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from poison import poisoned
from test_facility_sites import BBOXES, SITES, fixture_facilities, fixture_table, write_truth
from test_gpu_facilities import synthetic_run

from aquaculture_amd import facilities, facility_sites as fs, geocode

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
LENGTHS = [0, 1, 63, 64, 65, 129]


def dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()


def check_bounds(monkeypatch, start, box, use):
    from aquaculture_amd.engine import facility_bounds
    start, box, use = np.asarray(start, np.int32), np.asarray(box, np.float64).reshape(-1, 4), np.asarray(use, np.uint8)
    with poisoned(monkeypatch, 0xFF) as p:
        got = facility_bounds(dev(start, np.int32), dev(box, np.float64), dev(use, np.uint8), start)
        torch.cuda.synchronize()
        b = got.cpu().numpy()
        p.check_guards()
        assert not p.passed_through, p.passed_through
    want = fs.bounds_numpy(start, box, use)
    assert b.dtype == np.float64 and b.shape == want.shape and b.tobytes() == want.tobytes(), (b, want)
    return b


def check_joins(monkeypatch, qbox, qgroup, kbox, kgroup, G):
    """Both joins: counts, first rows, offsets and lists, equal to the restatements' byte for byte."""
    from aquaculture_amd.engine import box_join_count, box_join_list
    qbox, kbox = np.asarray(qbox, np.float64).reshape(-1, 4), np.asarray(kbox, np.float64).reshape(-1, 4)
    qgroup, kgroup = np.asarray(qgroup, np.int32), np.asarray(kgroup, np.int32)
    with poisoned(monkeypatch, 0xFF) as p:
        args = (dev(qbox, np.float64), dev(qgroup, np.int32), dev(kbox, np.float64), dev(kgroup, np.int32), G)
        c, f = box_join_count(*args)
        off, lst = box_join_list(*args, count=c)
        torch.cuda.synchronize()
        count, first, lst = c.cpu().numpy(), f.cpu().numpy(), lst.cpu().numpy()
        p.check_guards()
        assert not p.passed_through, p.passed_through
    want_c, want_f = fs.join_count_numpy(qbox, qgroup, kbox, kgroup, G)
    want_off, want_l = fs.join_list_numpy(qbox, qgroup, kbox, kgroup, G)
    assert count.dtype == np.int32 and count.tobytes() == want_c.tobytes(), (count, want_c)
    assert first.dtype == np.int32 and first.tobytes() == want_f.tobytes(), (first, want_f)
    assert off.dtype == np.int64 and off.tobytes() == want_off.tobytes(), (off, want_off)
    assert lst.dtype == np.int32 and lst.tobytes() == want_l.tobytes(), (lst, want_l)
    return count, first, off, lst


def random_boxes(r, n, span=40.0, size=12.0):
    a = r.uniform(0, span, (n, 2))
    return np.concatenate([a, a + r.uniform(0.5, size, (n, 2))], 1)


# ---- the bounds ----

@pytest.mark.parametrize("F", [1, 3, 5])
def test_bounds_part_filled_blocks(lib, monkeypatch, F):
    """A workgroup holds four wavefronts, one facility each: one, three and five facilities."""
    r = np.random.default_rng(F)
    sizes = r.integers(1, 90, F)
    start = np.concatenate([[0], np.cumsum(sizes)])
    b = check_bounds(monkeypatch, start, random_boxes(r, int(start[-1])), np.ones(int(start[-1]), np.uint8))
    assert np.isfinite(b).all()


@pytest.mark.parametrize("n", LENGTHS)
def test_bounds_entry_counts_at_the_lane_stride(lib, monkeypatch, n):
    """A facility of n entries between two others; one member is marked unused and holds the extremes, two hold NaNs."""
    r = np.random.default_rng(100 + n)
    box = random_boxes(r, 7 + n + 4)
    use = np.ones(box.shape[0], np.uint8)
    if n >= 1:
        box[7] = [-1000.0, -1000.0, 1000.0, 1000.0]
        use[7] = 0
    if n >= 63:
        box[7 + 5, 0], box[7 + 62, 3] = NAN, NAN
    b = check_bounds(monkeypatch, [0, 7, 7 + n, 11 + n], box, use)
    assert np.isfinite(b[[0, 2]]).all() and np.isnan(b[1]).all() == (n <= 1) and (n <= 1 or b[1, 0] > -1000.0)


@pytest.mark.parametrize("at", [0, 63, 64, 100])
def test_bounds_extreme_in_lane_0_lane_63_and_the_second_stride(lib, monkeypatch, at):
    r = np.random.default_rng(at)
    box = random_boxes(r, 130)
    box[at] = [-5.0, -6.0, 77.0, 78.0]
    b = check_bounds(monkeypatch, [0, 130], box, np.ones(130, np.uint8))
    assert b.tolist() == [[-5.0, -6.0, 77.0, 78.0]]


def test_bounds_unused_nan_infinite_and_signed_zeros(lib, monkeypatch):
    box = np.asarray([[0.0, -0.0, 1.0, 2.0], [-0.0, 0.0, 1.0, 2.0], [5.0, 5.0, INF, 6.0], [NAN, 1.0, 2.0, NAN], [1.0, 1.0, 2.0, 2.0], [3.0, 3.0, 4.0, 4.0],
                    [NAN, NAN, NAN, NAN], [7.0, 7.0, 8.0, 8.0]])
    b = check_bounds(monkeypatch, [0, 2, 3, 4, 4, 6, 8], box, [1, 1, 1, 1, 0, 0, 1, 1])
    assert np.signbit(b[0]).tolist() == [False, True, False, False]
    assert np.isnan(b[[1, 2, 3, 4]]).all() and b[5].tolist() == [7.0, 7.0, 8.0, 8.0]       # infinite, NaN alone, empty, all unused; a NaN member skipped
    check_bounds(monkeypatch, [0, 0, 0], np.zeros((0, 4)), np.zeros(0, np.uint8))           # no entry at all
    from aquaculture_amd.engine import facility_bounds
    got = facility_bounds(dev([0], np.int32), dev(box, np.float64), dev(np.ones(8), np.uint8), np.zeros(1, np.int32))
    assert got.shape == (0, 4)
    with pytest.raises(ValueError, match="entry_use"):
        facility_bounds(dev([0, 8], np.int32), dev(box, np.float64), dev(np.ones(8), np.int32), np.asarray([0, 8], np.int32))


# ---- the joins ----

@pytest.mark.parametrize("Q", [1, 3, 5])
def test_joins_part_filled_blocks(lib, monkeypatch, Q):
    r = np.random.default_rng(Q)
    count, _, _, _ = check_joins(monkeypatch, random_boxes(r, Q, size=30.0), np.zeros(Q, np.int32), random_boxes(r, 40), np.zeros(40, np.int32), 1)
    assert (count > 0).all()


def pattern_keys(r, N, match):
    """N keys of group 0 in a row along x, in a random row order, key at sorted position k inside the query's y range iff match[k]; and 7 keys
    of group 1 over the same ground."""
    x0 = np.arange(N) * 0.25
    y0 = np.where(np.asarray(match, bool), 1.0, 20.0)
    k = np.stack([x0, y0, x0 + 0.5, y0 + 1.0], 1).reshape(-1, 4)
    perm = r.permutation(N)                                 # row perm[i] holds position ... kbox[row] = k[position]
    other = np.stack([np.arange(7) * 4.0, np.full(7, 1.0), np.arange(7) * 4.0 + 3.0, np.full(7, 2.0)], 1)
    kbox = np.concatenate([other[:3], k[perm], other[3:]], 0)
    kgroup = np.concatenate([np.ones(3), np.zeros(N), np.ones(4)]).astype(np.int32)
    return kbox, kgroup, 3 + np.argsort(perm, kind="stable")      # rows in the order of the sorted run


PATTERNS = {"all": lambda N: np.ones(N, bool), "none": lambda N: np.zeros(N, bool), "alternating": lambda N: np.arange(N) % 2 == 0,
            "lane 63 of the first chunk": lambda N: np.arange(N) == 63, "lane 0 of the second chunk": lambda N: np.arange(N) == 64}


@pytest.mark.parametrize("N", LENGTHS)
@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_joins_run_lengths_and_match_patterns(lib, monkeypatch, N, name):
    """The edges of the lane stride, of the ballot and of its popcount prefix.  Query 0 spans the whole run, query 1 is the same box in the
    other group, query 2 lies beside everything, query 3 spans the run again: its list follows an empty one."""
    r = np.random.default_rng(1000 + N)
    match = PATTERNS[name](N)
    kbox, kgroup, rows = pattern_keys(r, N, match)
    q = [[-1.0, 0.0, 100.0, 3.0], [-1.0, 0.0, 100.0, 3.0], [200.0, 0.0, 201.0, 3.0], [-1.0, 1.5, 100.0, 1.75]]
    count, first, off, lst = check_joins(monkeypatch, q, [0, 1, 0, 0], kbox, kgroup, 2)
    want = rows[match].tolist()
    assert count.tolist() == [len(want), 7, 0, len(want)] and first[0] == (min(want) if want else -1) and first[2] == -1
    assert lst[off[0]:off[1]].tolist() == want and lst[off[3]:off[4]].tolist() == want and off[2] == off[3]


def test_joins_smallest_row_last_in_the_run(lib, monkeypatch):
    x0 = (130 - np.arange(130)) * 0.5                       # row 0 has the largest x0: it is the last key of the sorted run
    k = np.stack([x0, np.zeros(130), x0 + 2.0, np.full(130, 3.0)], 1)
    count, first, off, lst = check_joins(monkeypatch, [[-1.0, -1.0, 99.0, 9.0]], [0], k, np.zeros(130, np.int32), 1)
    assert count[0] == 130 and first[0] == 0 and lst.tolist() == list(range(129, -1, -1))


def test_joins_touching_nan_groups_out_of_range_and_the_group_border(lib, monkeypatch):
    k = np.array([[10.0, 0.0, 12.0, 5.0], [0.0, 10.0, 5.0, 12.0], [10.0, 10.0, 12.0, 12.0], [np.nextafter(10.0, INF), 0.0, 12.0, 5.0],
                  [1.0, NAN, 9.0, 9.0], [NAN, 0.0, 1.0, 1.0], [2.0, 2.0, 3.0, NAN], [4.0, 4.0, 5.0, 5.0]])
    q = np.array([[0.0, 0.0, 10.0, 10.0],                   # touches key 0 at an edge, key 1 at an edge, key 2 at a corner; holds key 7
                  [0.0, 0.0, np.nextafter(10.0, -INF), np.nextafter(10.0, -INF)],       # one ulp short of all three
                  [0.0, 0.0, NAN, 10.0], [NAN, NAN, NAN, NAN], [-INF, -INF, INF, INF], [4.5, 4.5, 4.5, 4.5]])
    count, first, _, _ = check_joins(monkeypatch, q, np.zeros(6, np.int32), k, np.zeros(8, np.int32), 1)
    assert count.tolist() == [4, 1, 0, 0, 5, 1] and first.tolist() == [0, 7, -1, -1, 0, 7]
    # group ids outside [0, G), a group without keys
    qq = np.tile(q[:1], (6, 1))
    count, first, _, lst = check_joins(monkeypatch, qq, [2, 3, -1, 4, 1 << 30, -(1 << 31)], k, np.zeros(8, np.int32), 4)
    assert (count == 0).all() and (first == -1).all() and lst.shape == (0,)
    # two groups over the same ground: a query only sees its own, on either side of the border between the runs
    kb = np.tile([[0.0, 0.0, 1.0, 1.0]], (140, 1)) + np.repeat(np.arange(70) * 0.01, 2)[:, None]
    kg = np.tile([0, 1], 70).astype(np.int32)
    count, first, off, lst = check_joins(monkeypatch, [[0.0, 0.0, 5.0, 5.0]] * 3, [0, 1, 2], kb, kg, 3)
    assert count.tolist() == [70, 70, 0] and first.tolist() == [0, 1, -1]
    assert lst[:70].tolist() == list(range(0, 140, 2)) and lst[70:].tolist() == list(range(1, 140, 2))


def test_joins_random_boxes_on_a_lattice_no_keys_and_no_queries(lib, monkeypatch):
    """Integer coordinates, so that touching edges are common; 5 groups, one of them without keys."""
    r = np.random.default_rng(11)

    def boxes(n):
        a, w = r.integers(0, 40, (n, 2)).astype(np.float64), r.integers(0, 5, (n, 2)).astype(np.float64)
        return np.concatenate([a, a + w], 1)

    q, k = boxes(700), boxes(900)
    qg, kg = r.integers(-1, 6, 700).astype(np.int32), r.choice([0, 1, 2, 4], 900).astype(np.int32)
    count, _, off, _ = check_joins(monkeypatch, q, qg, k, kg, 5)
    assert 100 < (count > 0).sum() < 690 and (count[(qg == 3) | (qg < 0) | (qg > 4)] == 0).all() and off[-1] > 700
    count, first, off, lst = check_joins(monkeypatch, q[:9], np.zeros(9, np.int32), np.zeros((0, 4)), np.zeros(0, np.int32), 1)
    assert (count == 0).all() and off.tolist() == [0] * 10
    _, _, off, lst = check_joins(monkeypatch, np.zeros((0, 4)), np.zeros(0, np.int32), k, kg, 5)
    assert off.tolist() == [0] and lst.shape == (0,)
    from aquaculture_amd import engine
    with pytest.raises(ValueError, match="group ids"):
        engine.box_join_count(dev(q, np.float64), dev(qg, np.int32), dev(k, np.float64), dev(kg, np.int32), 4)


def test_list_writes_stay_inside_the_querys_own_slice(lib):
    """Through the launcher itself, on a list filled with a sentinel: slices wider than the count keep their tail, the slice of a query
    without a match is untouched, and slices that are too short lose entries but nothing is written beside them."""
    from aquaculture_amd import engine
    r = np.random.default_rng(3)
    kbox, kgroup, rows = pattern_keys(r, 129, np.arange(129) % 3 != 1)
    q = np.asarray([[-1.0, 0.0, 100.0, 3.0], [200.0, 0.0, 201.0, 3.0], [-1.0, 1.5, 10.0, 1.75], [-1.0, 0.0, 100.0, 3.0]])
    qg = np.zeros(4, np.int32)
    off_want, lst_want = fs.join_list_numpy(q, qg, kbox, kgroup, 2)
    count = np.diff(off_want)
    assert count.tolist()[0] == 86 and count[1] == 0 and 0 < count[2] < 64
    keys = engine.box_join_keys(dev(kbox, np.float64), dev(kgroup, np.int32), 2)
    qd, gd = dev(q, np.float64), dev(qg, np.int32)
    stream = torch.cuda.current_stream().cuda_stream

    def run(offset):
        offset = np.ascontiguousarray(offset, dtype=np.int64)
        total = int(offset[-1]) + 5
        out, od = torch.full((total,), 0x77, dtype=torch.int32, device="cuda"), dev(offset, np.int64)
        rc = lib.aq_box_join_list_i32(qd.data_ptr(), gd.data_ptr(), 4, keys["box"].data_ptr(), keys["kid"].data_ptr(), keys["start"].data_ptr(),
                                      keys["start_host"].ctypes.data, keys["N"], keys["G"], od.data_ptr(), offset.ctypes.data, out.data_ptr(), total, stream)
        assert rc == 0, lib.aq_last_error()
        torch.cuda.synchronize()
        return out.cpu().numpy()

    wide = np.concatenate([[0], np.cumsum(count + 3)])     # three spare slots behind every list
    out = run(wide)
    for i in range(4):
        assert out[wide[i]:wide[i] + count[i]].tolist() == lst_want[off_want[i]:off_want[i + 1]].tolist(), i
        assert (out[wide[i] + count[i]:wide[i + 1]] == 0x77).all(), i
    assert (out[wide[4]:] == 0x77).all()
    short = np.concatenate([[0], np.cumsum(np.minimum(count, [70, 0, 1, 0]))])      # too few slots: 70 of 86, 1 of several, none of 86
    out = run(short)
    assert out[:70].tolist() == lst_want[:70].tolist() and out[70] == lst_want[off_want[2]] and (out[71:] == 0x77).all()


# ---- end to end ----

def read_all(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in (fs.GEOJSON_FILE, fs.CSV_FILE)}


def same_json(a, b):
    got, want = json.load(open(os.path.join(a, fs.JSON_FILE))), json.load(open(os.path.join(b, fs.JSON_FILE)))
    assert got["device"] != "cpu" and got["cpu"] is False and want["device"] == "cpu"
    assert {k: v for k, v in got.items() if k not in ("device", "cpu")} == {k: v for k, v in want.items() if k not in ("device", "cpu")}


def test_fixture_files_are_the_host_paths(lib, tmp_path):
    truth_path = write_truth(tmp_path / "truth.geojson")
    for name, truth in (("plain", None), ("truth", truth_path)):
        times = {}
        res = fs.facility_sites_from_table(fixture_facilities(), fixture_table(), SITES, BBOXES, str(tmp_path / name / "gpu"), truth, times=times)
        print({k: round(v, 3) for k, v in times.items()})
        assert set(times) == {"bounds_ms", "count_ms", "list_ms", "files_ms"} and times["bounds_ms"] > 0 and times["list_ms"] > 0
        want = fs.facility_sites_from_table(fixture_facilities(), fixture_table(), SITES, BBOXES, str(tmp_path / name / "cpu"), truth, cpu=True)
        assert read_all(tmp_path / name / "gpu") == read_all(tmp_path / name / "cpu")
        same_json(tmp_path / name / "gpu", tmp_path / name / "cpu")
        assert res["state"] == want["state"] and res["bounds"].tobytes() == want["bounds"].tobytes()
        assert (res["unique_additional_early"], res["unique_additional_late"]) == (7, 9) and res["state"].count("known") == 38


# ---- refusals ----

def test_bad_arguments_are_refused_and_nothing_is_launched(lib):
    stream = torch.cuda.current_stream().cuda_stream
    box = torch.tensor([[0.0, 0.0, 1.0, 1.0], [5.0, 5.0, 6.0, 7.0], [2.0, 2.0, 3.0, 3.0]], dtype=torch.float64, device="cuda")
    use = torch.ones(3, dtype=torch.uint8, device="cuda")
    start = torch.tensor([0, 2, 3], dtype=torch.int32, device="cuda")
    start_h = np.asarray([0, 2, 3], np.int32)
    out = torch.full((3, 4), -77.0, dtype=torch.float64, device="cuda")

    def bounds(s_h=start_h, F=2, E=3, s_p=start.data_ptr(), box_p=box.data_ptr(), use_p=use.data_ptr(), out_p=out.data_ptr()):
        return lib.aq_facility_bounds_f64(s_p, s_h.ctypes.data, F, box_p, use_p, E, out_p, stream)

    for kw, msg in (({"F": 1 << 31}, "2^31"), ({"E": -1}, "2^31"), ({"s_h": np.asarray([0, 3, 2], np.int32)}, "entry start"),
                    ({"s_h": np.asarray([0, 2, 4], np.int32)}, "entry start"), ({"box_p": None}, "null pointer"), ({"out_p": None}, "null pointer"),
                    ({"box_p": box.data_ptr() + 8}, "unaligned"), ({"s_p": start.data_ptr() + 2}, "unaligned")):
        assert bounds(**kw) == -1 and msg in lib.aq_last_error().decode(), (kw, lib.aq_last_error())
        torch.cuda.synchronize()
        assert bool((out == -77.0).all()), kw
    assert bounds(E=(1 << 31) - 1, box_p=None) == -1 and "null pointer" in lib.aq_last_error().decode()    # the largest count passes the size guard
    assert bounds() == 0
    torch.cuda.synchronize()
    assert out.tolist() == [[0.0, 0.0, 6.0, 7.0], [2.0, 2.0, 3.0, 3.0], [-77.0] * 4]

    q = torch.tensor([[0.0, 0.0, 1.0, 1.0], [5.0, 5.0, 6.0, 6.0]], dtype=torch.float64, device="cuda")
    qg = torch.zeros(2, dtype=torch.int32, device="cuda")
    kb = torch.tensor([[0.5, 0.5, 2.0, 2.0], [0.75, 0.0, 3.0, 3.0]], dtype=torch.float64, device="cuda")
    kid = torch.tensor([4, 3], dtype=torch.int32, device="cuda")
    gs = torch.tensor([0, 2], dtype=torch.int32, device="cuda")
    gs_h = np.asarray([0, 2], np.int32)
    count = torch.full((3,), 0x77, dtype=torch.int32, device="cuda")
    first = torch.full((3,), 0x77, dtype=torch.int32, device="cuda")
    lst = torch.full((4,), 0x77, dtype=torch.int32, device="cuda")
    off = torch.tensor([0, 2, 2], dtype=torch.int64, device="cuda")
    off_h = np.asarray([0, 2, 2], np.int64)

    def head(kw):
        return (kw.get("q_p", q.data_ptr()), kw.get("g_p", qg.data_ptr()), kw.get("Q", 2), kw.get("k_p", kb.data_ptr()), kw.get("id_p", kid.data_ptr()),
                kw.get("s_p", gs.data_ptr()), kw.get("s_h", gs_h).ctypes.data, kw.get("N", 2), kw.get("G", 1))

    def counts(**kw):
        return lib.aq_box_join_count_i32(*head(kw), kw.get("c_p", count.data_ptr()), kw.get("f_p", first.data_ptr()), stream)

    def lists(**kw):
        return lib.aq_box_join_list_i32(*head(kw), kw.get("o_p", off.data_ptr()), kw.get("o_h", off_h).ctypes.data, kw.get("l_p", lst.data_ptr()),
                                        kw.get("total", 2), stream)

    untouched = lambda: bool((count == 0x77).all()) and bool((first == 0x77).all()) and bool((lst == 0x77).all())
    common = (({"Q": 1 << 31}, "2^31"), ({"N": -1}, "2^31"), ({"G": 1 << 31}, "2^31"), ({"s_h": np.asarray([0, 3], np.int32)}, "group start"),
              ({"s_h": np.asarray([1, 0], np.int32)}, "group start"), ({"q_p": None}, "null pointer"), ({"id_p": None}, "null pointer"),
              ({"k_p": kb.data_ptr() + 16}, "unaligned"), ({"g_p": qg.data_ptr() + 2}, "unaligned"))
    for fn, extra in ((counts, (({"c_p": None}, "null pointer"), ({"f_p": first.data_ptr() + 2}, "unaligned"))),
                      (lists, (({"total": 1 << 31}, "2^31"), ({"o_h": np.asarray([0, 3, 2], np.int64)}, "offset"), ({"o_h": np.asarray([0, 2, 3], np.int64)}, "offset"),
                               ({"l_p": None}, "null pointer"), ({"o_p": off.data_ptr() + 4}, "unaligned")))):
        for kw, msg in common + extra:
            assert fn(**kw) == -1 and msg in lib.aq_last_error().decode(), (fn.__name__, kw, lib.aq_last_error())
            torch.cuda.synchronize()
            assert untouched(), (fn.__name__, kw)
    assert counts() == 0 and lists() == 0                   # and the same arguments, all valid, run
    torch.cuda.synchronize()
    assert count.tolist() == [2, 0, 0x77] and first.tolist() == [3, -1, 0x77] and lst.tolist() == [4, 3, 0x77, 0x77]


# ---- detect.py ----

def test_detect_py_writes_the_host_paths_files(lib, tmp_path):
    """The tiny sweep of tests/test_gpu_facilities.py's last test with --facility-sites and a truth file: the three files equal what the
    restatements make of the run's label files."""
    from PIL import Image
    from aquaculture_amd import checkpoint, tiles
    (tmp_path / "jpegs").mkdir()
    for k, i in enumerate((0, 3, 19, 20)):
        Image.fromarray(tiles.synthetic_tile(i, 640)).save(tmp_path / "jpegs" / f"ORTHOIMAGERY.ORTHOPHOTOS{2015 - k % 2}_3_{1024 * k}_0.jpeg", quality=95)
    checkpoint.write_synthetic_checkpoint(str(tmp_path / "synth.pt"), "yolov5m", 5)
    _, csv_path = synthetic_run(tmp_path)
    (x0, y0, x1, y1), = geocode.load_wanted_bboxes(csv_path).values()
    lon, lat = geocode.mercator_to_lonlat(np.asarray([x0 + 150.0, x0 + 1500.0, x1 + 5000.0]), np.asarray([y1 - 150.0, y0 + 100.0, y0]))
    sites = tmp_path / "sites.csv"
    sites.write_text("lat,lon,num_cages\n" + "".join(f"{a!r},{o!r},{n}\n" for a, o, n in zip(lat.tolist(), lon.tolist(), (60, 7, 3))))
    from test_gpu_model_errors import tiled_truth
    truth_path = tiled_truth(tmp_path / "truth.geojson", csv_path)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "yolov5", "detect.py"), "--weights", str(tmp_path / "synth.pt"), "--source",
                        str(tmp_path / "jpegs"), "--save-txt", "--save-conf", "--nosave", "--project", str(tmp_path / "runs"), "--name", "fs",
                        "--batch-size", "4", "--geocode-bboxes", csv_path, "--facilities", "--facilities-conf", "0.25", "--facilities-eps", "25",
                        "--facilities-min-cages", "4", "--facilities-by", "pass", "--facility-sites", str(sites), "--facility-sites-truth", truth_path],
                       capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    run = tmp_path / "runs" / "fs"
    print(" ".join(l for l in (r.stdout + r.stderr).splitlines() if "facility sites" in l))
    assert "facility_sites" not in json.load(open(run / "run_params.json"))
    table = geocode.geocode_label_dir(str(run / "labels"), csv_path)
    fac = facilities.cluster(table, "pass", 0.25, 25.0, 4, 640, 640, labels_fn=facilities.dbscan_numpy)
    want = fs.facility_sites_from_table(fac, table, str(sites), csv_path, str(tmp_path / "want"), truth_path, cpu=True)
    assert read_all(run) == read_all(tmp_path / "want")
    same_json(run, tmp_path / "want")
    assert fs.describe(want) in r.stdout + r.stderr and len(want["pass"]) >= 1 and want["sites"]["box"].shape[0] == 2 and want["sites"]["read"] == 3
