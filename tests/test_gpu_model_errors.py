"""--model-errors on the GPU: aq_model_error_match_f64 and aq_model_error_moments_f64 (csrc/model_errors.hip) through
engine.model_error_match / engine.model_error_moments against the numpy restatement (model_errors.match_numpy, moments_numpy), bit for bit
(``tobytes()``: NaN payloads included), every output between poisoned guard regions; the lane-stride edges of the match, its tie rule across
and within lanes, the written order of the moments; the fixture of tests/test_model_errors.py end to end; the launchers' refusals; one
detect.py run in a child process under its own time limit."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from poison import poisoned
from test_gpu_facilities import synthetic_run
from test_model_errors import CONF, detection_table, fixture_match, fixture_samples, truth_feature, write_features, write_truth_geojson

from aquaculture_amd import geocode, model_errors, tonnage

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


def dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()


def check_match(monkeypatch, qbox, qgroup, kbox, kgroup, G, qarea=None, karea=None):
    """The kernel's three outputs, equal to the restatement's byte for byte; allocated poisoned (0xFF) and between guards."""
    from aquaculture_amd.engine import model_error_match
    qbox, kbox = np.asarray(qbox, np.float64).reshape(-1, 4), np.asarray(kbox, np.float64).reshape(-1, 4)
    qgroup, kgroup = np.asarray(qgroup, np.int32), np.asarray(kgroup, np.int32)
    qarea = np.linspace(1.0, 2.0, qbox.shape[0]) if qarea is None else np.asarray(qarea, np.float64)
    karea = np.linspace(50.0, 90.0, kbox.shape[0]) if karea is None else np.asarray(karea, np.float64)
    with poisoned(monkeypatch, 0xFF) as p:
        got = model_error_match(dev(qbox, np.float64), dev(qgroup, np.int32), dev(qarea, np.float64), dev(kbox, np.float64), dev(kgroup, np.int32),
                                dev(karea, np.float64), G)
        torch.cuda.synchronize()
        match, overlap, error = (t.cpu().numpy() for t in got)
        p.check_guards()
        assert not p.passed_through, p.passed_through
    want = model_errors.match_numpy(qbox, qgroup, qarea, kbox, kgroup, karea)
    assert match.dtype == np.int32 and overlap.dtype == np.float64 and error.dtype == np.float64
    assert match.tobytes() == want[0].tobytes(), np.nonzero(match != want[0])[0][:10]
    assert overlap.tobytes() == want[1].tobytes(), (overlap[:8], want[1][:8])
    assert error.tobytes() == want[2].tobytes(), (error[:8], want[2][:8])
    return match, overlap, error


def check_moments(monkeypatch, error, match, mgroup, G):
    from aquaculture_amd.engine import model_error_moments
    error, match, mgroup = np.asarray(error, np.float64), np.asarray(match, np.int32), np.asarray(mgroup, np.int32)
    with poisoned(monkeypatch, 0xFF) as p:
        got = model_error_moments(dev(error, np.float64), dev(match, np.int32), dev(mgroup, np.int32), G)
        torch.cuda.synchronize()
        n, mean, sd = (t.cpu().numpy() for t in got)
        p.check_guards()
        assert not p.passed_through, p.passed_through
    want = model_errors.moments_numpy(error, match, mgroup, G)
    assert n.dtype == np.int64 and n.tobytes() == want[0].tobytes(), (n, want[0])
    assert mean.tobytes() == want[1].tobytes(), (mean, want[1])
    assert sd.tobytes() == want[2].tobytes(), (sd, want[2])
    return n, mean, sd


def random_boxes(r, n, span=40.0, size=12.0):
    a = r.uniform(0, span, (n, 2))
    return np.concatenate([a, a + r.uniform(0.5, size, (n, 2))], 1)


# ---- the match ----

@pytest.mark.parametrize("Q", [1, 3, 5])
def test_match_part_filled_blocks(lib, monkeypatch, Q):
    """A workgroup holds four wavefronts, one query each: one, three and five queries."""
    r = np.random.default_rng(Q)
    k = random_boxes(r, 40)
    m, _, _ = check_match(monkeypatch, random_boxes(r, Q, size=30.0), np.zeros(Q, np.int32), k, np.zeros(40, np.int32), 1)
    assert (m >= 0).all()


@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 129])
def test_match_run_lengths_at_the_lane_stride(lib, monkeypatch, N):
    """N candidates in the query's group (all of them meet it, with distinct intersections), 7 keys in another group beside them."""
    r = np.random.default_rng(100 + N)
    x0 = r.permutation(N) * 0.25
    k = np.stack([x0, np.zeros(N), x0 + 1.0 + r.permutation(N) * 0.01, np.full(N, 5.0)], 1).reshape(-1, 4)
    other = random_boxes(r, 7)
    kbox, kgroup = np.concatenate([other[:3], k, other[3:]], 0), np.concatenate([np.ones(3), np.zeros(N), np.ones(4)]).astype(np.int32)
    q = [[-1.0, 1.0, 100.0, 4.0], [-1.0, 1.0, 100.0, 4.0], [10.0, 10.0, 11.0, 11.0]]
    m, _, _ = check_match(monkeypatch, q, [0, 1, 0], kbox, kgroup, 2)
    if N:
        assert m[0] == 3 + int(np.argmax(k[:, 2] - k[:, 0])) and m[2] == -1
    else:
        assert m[0] == -1 and m[2] == -1
    assert m[1] in (-1, 0, 1, 2, 3 + N, 4 + N, 5 + N, 6 + N)


@pytest.mark.parametrize("at", [0, 63, 64, 100])
def test_match_winner_in_lane_0_lane_63_and_the_second_stride(lib, monkeypatch, at):
    """130 keys in x order, all inside the query; the one at sorted position `at` is taller than the others.  Rows are a permutation, so
    the row written is not the position."""
    r = np.random.default_rng(at)
    x0 = np.arange(130) * 0.5
    k = np.stack([x0, np.zeros(130), x0 + 2.0, np.full(130, 3.0)], 1)
    k[at, 3] = 4.0
    perm = r.permutation(130)
    m, ov, _ = check_match(monkeypatch, [[-1.0, -1.0, 99.0, 9.0]], [0], k[perm], np.zeros(130, np.int32), 1)
    assert perm[m[0]] == at and ov[0] == 100.0 * 8.0 / 1000.0


def test_match_equal_intersections_across_lanes_and_within_one(lib, monkeypatch):
    x0 = np.arange(130) * 0.5
    base = np.stack([x0, np.zeros(130), x0 + 2.0, np.full(130, 3.0)], 1)
    q = [[-1.0, -1.0, 99.0, 9.0]]
    r = np.random.default_rng(2)
    # every key the same intersection: the smallest row wins wherever the sort has put it
    for _ in range(3):
        m, _, _ = check_match(monkeypatch, q, [0], base[r.permutation(130)], np.zeros(130, np.int32), 1)
        assert m[0] == 0
    # two taller keys with the same intersection, in one lane (positions 3 and 67) and in two lanes (3 and 40); either may hold the smaller row
    for a, b in ((3, 67), (3, 40), (0, 64), (63, 127), (62, 129)):
        k = base.copy()
        k[[a, b], 3] = 4.0
        for first in (a, b):
            perm = np.concatenate([[first], [a + b - first], np.delete(np.arange(130), [a, b])])        # perm[row] = position: rows 0 and 1 are the two
            m, _, _ = check_match(monkeypatch, q, [0], k[perm], np.zeros(130, np.int32), 1)
            assert m[0] == 0 and perm[0] == first
    # identical boxes (the same x0: the sort keeps their order)
    m, _, _ = check_match(monkeypatch, q, [0], np.repeat(base[:1], 70, 0), np.zeros(70, np.int32), 1)
    assert m[0] == 0


def test_match_touching_runs_groups_out_of_range_nan_and_boxes_without_area(lib, monkeypatch):
    # an all-touching run: 70 keys on the query's upper edge, every intersection 0
    x0 = np.arange(70) * 0.1
    touching = np.stack([x0, np.full(70, 10.0), x0 + 1.0, np.full(70, 12.0)], 1)
    r = np.random.default_rng(4)
    perm = r.permutation(70)
    m, ov, _ = check_match(monkeypatch, [[0.0, 0.0, 10.0, 10.0]], [0], touching[perm], np.zeros(70, np.int32), 1)
    assert m[0] == 0 and ov[0] == 0.0
    # ... and one that overlaps among them wins
    k = touching[perm].copy()
    k[55] = [1.0, 9.0, 2.0, 12.0]
    m, ov, _ = check_match(monkeypatch, [[0.0, 0.0, 10.0, 10.0]], [0], k, np.zeros(70, np.int32), 1)
    assert m[0] == 55 and ov[0] == 1.0
    # group ids outside [0, G), a group without keys
    q = np.tile([[0.0, 0.0, 10.0, 10.0]], (6, 1))
    m, ov, err = check_match(monkeypatch, q, [2, 3, -1, 4, 1 << 30, -(1 << 31)], k, np.zeros(70, np.int32), 4)
    assert (m == -1).all() and np.isnan(ov).all() and np.isnan(err).all()
    # NaN queries, NaN keys, a NaN area on either side, unbounded boxes whose intersection is inf x 0
    k = np.array([[1.0, NAN, 9.0, 9.0], [4.0, 4.0, 5.0, 5.0], [NAN, 0.0, 1.0, 1.0], [0.0, 10.0, INF, 20.0], [0.0, 10.0, 5.0, 20.0], [2.0, 2.0, 3.0, NAN]])
    q = np.array([[0.0, 0.0, NAN, 10.0], [0.0, 0.0, 10.0, 10.0], [NAN, NAN, NAN, NAN], [0.0, 0.0, INF, 10.0], [5.0, 11.0, INF, 12.0], [4.5, 4.5, 4.5, 4.5],
                  [5.0, 5.0, 5.0, 7.0], [-INF, -INF, INF, INF]])
    m, ov, err = check_match(monkeypatch, q, np.zeros(8, np.int32), k, np.zeros(6, np.int32), 1, qarea=[1, 2, 3, 4, 5, NAN, 7, 8],
                             karea=[10, 20, 30, NAN, 50, 60])
    assert m.tolist() == [-1, 1, -1, 1, 3, 1, 1, 3]
    # a query without area: 0 / 0 is the canonical NaN, and the area difference of a NaN area too
    assert ov[5:7].tobytes() == np.array([np.nan, np.nan]).tobytes() and err[5:6].tobytes() == np.array([np.nan]).tobytes() and err[6] == 13.0
    assert ov[4] == INF or np.isnan(ov[4])


def test_match_random_boxes_on_a_lattice_and_the_fixture(lib, monkeypatch):
    """Integer coordinates, so that equal intersections and touching edges are common; 5 groups, one of them without keys."""
    r = np.random.default_rng(11)

    def boxes(n):
        a, w = r.integers(0, 40, (n, 2)).astype(np.float64), r.integers(0, 5, (n, 2)).astype(np.float64)
        return np.concatenate([a, a + w], 1)

    q, k = boxes(700), boxes(900)
    qg, kg = r.integers(-1, 6, 700).astype(np.int32), r.choice([0, 1, 2, 4], 900).astype(np.int32)
    m, _, _ = check_match(monkeypatch, q, qg, k, kg, 5, qarea=r.uniform(1, 2, 700), karea=r.uniform(1, 2, 900))
    assert 100 < (m >= 0).sum() < 690 and (m[(qg == 3) | (qg < 0) | (qg > 4)] == -1).all()
    s = fixture_samples()
    m, ov, err = check_match(monkeypatch, s["q"]["box"], s["q"]["group"], s["k"]["box"], s["k"]["group"], s["G"], s["q"]["area"], s["k"]["area"])
    want = fixture_match()
    assert m.tobytes() == want[0].tobytes() and ov.tobytes() == want[1].tobytes() and err.tobytes() == want[2].tobytes()
    from aquaculture_amd.engine import model_error_match
    e = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")
    got = model_error_match(e(0, 4), torch.zeros(0, dtype=torch.int32, device="cuda"), e(0), dev(k, np.float64), dev(kg, np.int32), e(900), 5)
    assert [t.shape for t in got] == [(0,)] * 3


# ---- the moments ----

@pytest.mark.parametrize("members", [0, 1, 63, 64, 65, 4097])
def test_moments_member_counts_at_the_lane_stride(lib, monkeypatch, members):
    """Group 0 has `members` members and group 1 members + 2, interleaved row by row; between them unmatched rows, rows of no group, rows
    whose error is not finite, and -0.0 among the members.  Group 2 stays empty."""
    r = np.random.default_rng(members)
    rows = []
    for i in range(members + 2):
        if i < members:
            rows.append((r.normal(3.0, 40.0) * 10.0 ** r.integers(-3, 4), 5, 0))
        rows.append((r.normal(-2.0, 10.0), 0, 1))
        if i % 3 == 0:
            rows.append((r.normal(), -1, i % 2))          # unmatched
        if i % 5 == 0:
            rows.append(((NAN, INF, -INF)[i % 3], 7, i % 2))   # not finite
        if i % 7 == 0:
            rows.append((1.0e9, 3, (-1, 3, 1 << 30)[i % 3]))   # no group
        if i % 4 == 0:
            rows.append((-0.0, 2, i % 2))
    error, match, mgroup = (np.asarray([row[j] for row in rows], dt) for j, dt in enumerate((np.float64, np.int32, np.int32)))
    n, mean, sd = check_moments(monkeypatch, error, match, mgroup, 3)
    extra = lambda g: sum(1 for i in range(members + 2) if i % 4 == 0 and i % 2 == g)
    assert n.tolist() == [members + extra(0), members + 2 + extra(1), 0] and np.isnan(mean[2]) and np.isnan(sd[2])
    assert np.isfinite(mean[1]) and sd[1] > 0


def test_moments_signed_zeros_one_member_and_no_rows(lib, monkeypatch):
    n, mean, sd = check_moments(monkeypatch, [-0.0, -0.0, 5.0, -0.0], [0, 0, 0, 0], [0, 0, 1, 2], 4)
    assert n.tolist() == [2, 1, 1, 0] and mean[:3].tolist() == [0.0, 5.0, 0.0] and sd[:3].tolist() == [0.0, 0.0, 0.0]
    check_moments(monkeypatch, np.zeros(0), np.zeros(0, np.int32), np.zeros(0, np.int32), 2)
    check_moments(monkeypatch, [1.0e308, 1.0e308, 1.0], [0, 0, 0], [0, 0, 0], 1)             # the sum overflows: inf, and the sd with it
    from aquaculture_amd.engine import model_error_moments
    got = model_error_moments(dev([1.0], np.float64), dev([0], np.int32), dev([0], np.int32), 0)
    assert [t.shape for t in got] == [(0,)] * 3


# ---- end to end ----

def test_fixture_files_are_the_host_paths(lib, tmp_path):
    table = detection_table()
    truth_path = write_truth_geojson(str(tmp_path / "truth.geojson"))
    times = {}
    res = model_errors.model_errors_from_table(table, truth_path, str(tmp_path / "gpu"), CONF, times=times)
    print({k: round(v, 3) for k, v in times.items()})
    assert set(times) == {"sort_ms", "kernel_ms", "files_ms"} and times["kernel_ms"] > 0
    want = model_errors.model_errors_from_table(table, truth_path, str(tmp_path / "cpu"), CONF, cpu=True)
    for f in (model_errors.CSV_FILE, model_errors.CAGES_FILE):
        assert open(tmp_path / "gpu" / f, "rb").read() == open(tmp_path / "cpu" / f, "rb").read(), f
    got_s, want_s = (json.load(open(tmp_path / d / model_errors.JSON_FILE)) for d in ("gpu", "cpu"))
    assert got_s["device"] != "cpu" and got_s["cpu"] is False
    assert {k: v for k, v in got_s.items() if k not in ("device", "cpu")} == {k: v for k, v in want_s.items() if k not in ("device", "cpu")}
    assert res["errors"] == want["errors"] and len(res["errors"]) >= 6 and res["n_matched"] > 950


# ---- refusals ----

def test_bad_arguments_are_refused_and_nothing_is_launched(lib):
    stream = torch.cuda.current_stream().cuda_stream
    q = torch.tensor([[0.0, 0.0, 1.0, 1.0], [5.0, 5.0, 6.0, 6.0]], dtype=torch.float64, device="cuda")
    qg = torch.zeros(2, dtype=torch.int32, device="cuda")
    qa = torch.tensor([1.0, 2.0], dtype=torch.float64, device="cuda")
    kb = torch.tensor([[0.5, 0.5, 2.0, 2.0], [0.0, 0.0, 0.0, 0.0]], dtype=torch.float64, device="cuda")[:1]
    kr = torch.zeros(2, dtype=torch.int32, device="cuda")
    ka = torch.tensor([4.0, 0.0], dtype=torch.float64, device="cuda")
    start = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    match = torch.full((2,), 0x77, dtype=torch.int32, device="cuda")
    ov = torch.full((2,), -77.0, dtype=torch.float64, device="cuda")
    err = torch.full((3,), -77.0, dtype=torch.float64, device="cuda")

    def call(q_p=q.data_ptr(), qg_p=qg.data_ptr(), qa_p=qa.data_ptr(), Q_=2, k_p=kb.data_ptr(), kr_p=kr.data_ptr(), ka_p=ka.data_ptr(), N_=1,
             start_p=start.data_ptr(), G_=1, m_p=match.data_ptr(), ov_p=ov.data_ptr(), err_p=err.data_ptr()):
        return lib.aq_model_error_match_f64(q_p, qg_p, qa_p, Q_, k_p, kr_p, ka_p, N_, start_p, G_, m_p, ov_p, err_p, stream)

    untouched = lambda: bool((match == 0x77).all()) and bool((ov == -77.0).all()) and bool((err == -77.0).all())
    for kw, msg in (({"Q_": 1 << 31}, "2\\^31"), ({"N_": 1 << 31}, "2\\^31"), ({"Q_": -1}, "2\\^31"), ({"N_": -1}, "2\\^31"), ({"G_": -1}, "groups"),
                    ({"q_p": None}, "null pointer"), ({"qg_p": None}, "null pointer"), ({"qa_p": None}, "null pointer"), ({"k_p": None}, "null pointer"),
                    ({"kr_p": None}, "null pointer"), ({"ka_p": None}, "null pointer"), ({"start_p": None}, "null pointer"),
                    ({"m_p": None}, "null pointer"), ({"ov_p": None}, "null pointer"), ({"err_p": None}, "null pointer"),
                    ({"q_p": q.data_ptr() + 16}, "unaligned"), ({"k_p": kb.data_ptr() + 8}, "unaligned"), ({"qa_p": qa.data_ptr() + 4}, "unaligned"),
                    ({"kr_p": kr.data_ptr() + 2}, "unaligned"), ({"ka_p": ka.data_ptr() + 4}, "unaligned"), ({"m_p": match.data_ptr() + 2}, "unaligned"),
                    ({"err_p": err.data_ptr() + 4}, "unaligned")):
        assert call(**kw) == -1, kw
        assert re.search(msg, lib.aq_last_error().decode()), (kw, lib.aq_last_error())
        torch.cuda.synchronize()
        assert untouched(), kw
    assert call(Q_=(1 << 31) - 1, q_p=None) == -1 and "null pointer" in lib.aq_last_error().decode()      # the largest count passes the size guard
    assert lib.aq_model_error_match_f64(None, None, None, 0, None, None, None, 0, None, 0, None, None, None, stream) == 0        # Q = 0 does nothing

    n = torch.full((2,), 0x77, dtype=torch.int64, device="cuda")
    mean = torch.full((2,), -77.0, dtype=torch.float64, device="cuda")
    sd = torch.full((3,), -77.0, dtype=torch.float64, device="cuda")
    e_in = torch.tensor([1.0, 3.0], dtype=torch.float64, device="cuda")
    m_in = torch.zeros(2, dtype=torch.int32, device="cuda")
    g_in = torch.tensor([0, 0], dtype=torch.int32, device="cuda")

    def moments(e_p=e_in.data_ptr(), m_p=m_in.data_ptr(), g_p=g_in.data_ptr(), Q_=2, G_=2, n_p=n.data_ptr(), mean_p=mean.data_ptr(), sd_p=sd.data_ptr()):
        return lib.aq_model_error_moments_f64(e_p, m_p, g_p, Q_, G_, n_p, mean_p, sd_p, stream)

    clean = lambda: bool((n == 0x77).all()) and bool((mean == -77.0).all()) and bool((sd == -77.0).all())
    for kw, msg in (({"Q_": 1 << 31}, "2\\^31"), ({"G_": 1 << 31}, "2\\^31"), ({"Q_": -1}, "2\\^31"), ({"G_": -1}, "2\\^31"),
                    ({"e_p": None}, "null pointer"), ({"m_p": None}, "null pointer"), ({"g_p": None}, "null pointer"), ({"n_p": None}, "null pointer"),
                    ({"mean_p": None}, "null pointer"), ({"sd_p": None}, "null pointer"), ({"e_p": e_in.data_ptr() + 4}, "unaligned"),
                    ({"g_p": g_in.data_ptr() + 2}, "unaligned"), ({"n_p": n.data_ptr() + 4}, "unaligned"), ({"sd_p": sd.data_ptr() + 4}, "unaligned")):
        assert moments(**kw) == -1, kw
        assert re.search(msg, lib.aq_last_error().decode()), (kw, lib.aq_last_error())
        torch.cuda.synchronize()
        assert clean(), kw
    assert moments(G_=(1 << 31) - 1, n_p=None) == -1 and "null pointer" in lib.aq_last_error().decode()
    assert lib.aq_model_error_moments_f64(None, None, None, 0, 0, None, None, None, stream) == 0                                 # G = 0 does nothing
    from aquaculture_amd import engine
    with pytest.raises(ValueError, match="group ids"):
        engine.model_error_match(q, qg, qa, kb, torch.tensor([1], dtype=torch.int32, device="cuda"), ka[:1], 1)
    torch.cuda.synchronize()
    assert untouched() and clean()
    assert call() == 0 and moments() == 0                   # and the same arguments, all valid, run
    torch.cuda.synchronize()
    assert match.tolist() == [0, -1] and ov[0].item() == 25.0 and err[0].item() == 3.0 and err[2].item() == -77.0
    assert n.tolist() == [2, 0] and mean[0].item() == 2.0 and sd[0].item() == 1.0 and sd[2].item() == -77.0


# ---- detect.py ----

def tiled_truth(path, csv_path, years=(2015, 2014)):
    """Labels that cover scene 3 of synthetic_run's bounds table without a gap: 70 m squares, a circle_cage and a square_cage on each, in each
    of `years`; every label carries its pixel box, one column of them at the image's left border."""
    (x0, y0, x1, y1), = geocode.load_wanted_bboxes(csv_path).values()
    feats = []
    for year in years:
        for i in range(20):
            for j in range(6):
                a, b = x0 + 70.0 * i, y1 - 70.0 * (j + 1)
                for ty in ("circle_cage", "square_cage"):
                    feats.append(truth_feature(a, b, a + 70.0, b + 70.0, ty, year, f"ORTHOIMAGERY.ORTHOPHOTOS{year}_3_{1024 * (i // 4)}_0.jpeg",
                                               px=(0.0 if i % 4 == 0 else 233.0 * (i % 4), 233.0 * j, 233.0 * (i % 4 + 1), 233.0 * (j + 1))))
    return write_features(path, feats)


def test_detect_py_hands_its_model_errors_to_the_bootstrap(lib, tmp_path):
    """The tiny sweep of tests/test_gpu_tonnage.py's last test with --model-errors --tonnage: the three model-error files equal what the
    restatement makes of the run's label files, and the bootstrap ran with that table: tonnage.json names it and the estimates are those of
    a run that reads model_errors.csv as --tonnage-errors."""
    from PIL import Image
    from aquaculture_amd import checkpoint, tiles
    (tmp_path / "jpegs").mkdir()
    for k, i in enumerate((0, 3, 19, 20)):
        Image.fromarray(tiles.synthetic_tile(i, 640)).save(tmp_path / "jpegs" / f"ORTHOIMAGERY.ORTHOPHOTOS{2015 - k % 2}_3_{1024 * k}_0.jpeg", quality=95)
    checkpoint.write_synthetic_checkpoint(str(tmp_path / "synth.pt"), "yolov5m", 5)
    _, csv_path = synthetic_run(tmp_path)
    truth_path = tiled_truth(tmp_path / "truth.geojson", csv_path)
    (tmp_path / "factors.csv").write_text("pass,s_mean,s_sd,h_mean,h_sd\n2013-2015,12,3,0.8,0.1\n")
    factors = str(tmp_path / "factors.csv")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "yolov5", "detect.py"), "--weights", str(tmp_path / "synth.pt"), "--source",
                        str(tmp_path / "jpegs"), "--save-txt", "--save-conf", "--nosave", "--project", str(tmp_path / "runs"), "--name", "me",
                        "--batch-size", "4", "--geocode-bboxes", csv_path, "--facilities-conf", "0.25", "--facilities-eps", "25",
                        "--facilities-min-cages", "4", "--model-errors", truth_path, "--tonnage", "--tonnage-factors", factors, "--tonnage-K", "200"],
                       capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    run = tmp_path / "runs" / "me"
    print(" ".join(l for l in (r.stdout + r.stderr).splitlines() if "model errors" in l))
    assert "model_errors" not in json.load(open(run / "run_params.json"))
    table = geocode.geocode_label_dir(str(run / "labels"), csv_path)
    want = model_errors.model_errors_from_table(table, truth_path, str(tmp_path / "want"), 0.25, cpu=True, widths=640, heights=640)
    for f in (model_errors.CSV_FILE, model_errors.CAGES_FILE):
        assert open(run / f, "rb").read() == open(tmp_path / "want" / f, "rb").read(), f
    s = json.load(open(run / model_errors.JSON_FILE))
    assert s["conf"] == 0.25 and s["device"] != "cpu" and s["n_matched"] == want["n_matched"] >= 4 and len(want["errors"]) >= 1
    assert model_errors.describe(want) in r.stdout + r.stderr
    doc = json.load(open(run / tonnage.JSON_FILE))
    assert doc["errors"] == [[*k, *v] for k, v in sorted(want["errors"].items())] and doc["errors"]
    by_file = tonnage.tonnage_from_table(table, str(tmp_path / "ton"), factors, str(run / model_errors.CSV_FILE), K=200, conf_thresh=0.25, eps=25.0,
                                         min_cages=4, widths=640, heights=640, cpu=True)
    assert len(by_file["facility_index"]) >= 1
    for f in (tonnage.ESTIMATES_FILE, tonnage.FACILITIES_FILE):
        assert open(run / f, "rb").read() == open(tmp_path / "ton" / f, "rb").read(), f
