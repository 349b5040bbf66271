"""--evaluate-kfold on the GPU: aq_eval_member_conf_subsets_f64 and aq_box_match_subsets_f64 (csrc/eval_subsets.hip) through
engine.eval_member_conf_subsets / engine.box_match_subsets against the numpy restatements, bit for bit; under the poisoned allocator; their
refusals through the C ABI; the cross-validation's three files against the host path's, and the two command lines in child processes under
their own time limits.  Shapes are the smallest at which the kernels can go wrong."""
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from poison import poisoned
from test_evaluate import SMALL_GRID, detection_table, fixture_data, truth
from test_facilities import CASES, TIE
from test_gpu_evaluate import GRID_ARGS, GRIDS, confidences, lattice_truth, match_gpu, member_gpu
from test_gpu_facilities import synthetic_run
from test_kfold import kfold_inputs, subset_masks

from aquaculture_amd import evaluate, geocode, kfold

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG_INF = float("-inf")
dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()


def words(mask):
    """uint32 words as the int64 tensor the bindings take."""
    return dev(np.asarray(mask).astype(np.int64), np.int64)


def member_subsets_gpu(xy, group, conf, mask, eps, K, S):
    from aquaculture_amd.engine import eval_member_conf_subsets
    return eval_member_conf_subsets(dev(xy, np.float64), dev(group, np.int32), dev(conf, np.float64), words(mask), eps, K, S)


def check_member(xy, group, conf, mask, eps, K, S):
    got = member_subsets_gpu(xy, group, conf, mask, eps, K, S).cpu()
    want = torch.from_numpy(kfold.member_conf_subsets_numpy(xy, group, conf, mask, eps, K, S))
    assert got.dtype == torch.float64 and got.shape == (S, xy.shape[0], K)
    assert torch.equal(got, want), np.argwhere(got.numpy() != want.numpy())[:10]
    return got.numpy()


def match_subsets_gpu(qbox, qgroup, qmask, kbox, kgroup, kmask, G, S, payload=None):
    from aquaculture_amd.engine import box_match_subsets
    hit, out = box_match_subsets(dev(np.reshape(qbox, (-1, 4)), np.float64), dev(qgroup, np.int32), words(qmask), dev(np.reshape(kbox, (-1, 4)), np.float64),
                                 dev(kgroup, np.int32), words(kmask), G, S, None if payload is None else dev(payload, np.float64))
    assert hit.dtype == torch.int32 and (out is None) == (payload is None)
    return hit.cpu().numpy().view(np.uint32), None if out is None else out.cpu().numpy()


def check_match(qbox, qgroup, qmask, kbox, kgroup, kmask, G, S, payload=None):
    hit, out = match_subsets_gpu(qbox, qgroup, qmask, kbox, kgroup, kmask, G, S, payload)
    want_hit, want_out = kfold.box_match_subsets_numpy(np.reshape(qbox, (-1, 4)), qgroup, qmask, np.reshape(kbox, (-1, 4)), kgroup, kmask, S, payload)
    assert np.array_equal(hit, want_hit), np.nonzero(hit != want_hit)[0][:10]
    if payload is not None:
        assert out.dtype == np.float64 and out.shape == want_out.shape and np.array_equal(out, want_out), np.argwhere(out != want_out)[:10]
    return hit, out


# ---- eval_member_conf_subsets ----

@pytest.mark.parametrize("S", [1, 12, 32])
@pytest.mark.parametrize("K", [1, 10, 16])
def test_member_conf_subsets_is_the_host_restatements_bit_for_bit(lib, K, S):
    for name in ("four_coincident", "one_point", "blobs_0", "cell_edges", "two_groups"):
        xy, group, eps, _ = CASES[name]
        n = xy.shape[0]
        M = check_member(xy, group, confidences(n, 7), subset_masks(n, S, 3), eps, K, S)
        if S > 1:
            assert (M[0] == NEG_INF).all()                  # the empty subset; bit S - 1 (bit 31 with S = 32) holds all points but the first two
            if n > 2:
                assert np.isfinite(M[S - 1, 2:, 0]).all() and (M[S - 1, :2] == NEG_INF).all()
    xy, group, eps, _ = TIE                                 # every step of the row is exactly eps
    conf = np.array([0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.95, 0.99])
    M = check_member(xy, group, conf, np.full(8, (1 << S) - 1, np.uint32), eps, K, S)
    if K >= 3:
        assert M[S - 1, :6, 2].tolist() == [0.7, 0.7, 0.7, 0.6, 0.5, 0.4] and M[S - 1, 6:, 2].tolist() == [NEG_INF, NEG_INF]
    # without point 2 the row falls apart: what bit s says changes the neighbourhoods, not only the rows
    mask = np.full(8, (1 << S) - 1, np.uint32)
    mask[2] = 0
    M = check_member(xy, group, conf, mask, eps, K, S)
    if K >= 3:
        assert M[0, :6, 2].tolist() == [NEG_INF, NEG_INF, NEG_INF, 0.4, 0.4, 0.4]        # 3, 4, 5 are left: only 4 sees three points


def test_member_conf_subsets_across_a_workgroup_edge_of_the_fixture_and_twice(lib):
    r = np.random.default_rng(4)
    xy, group = r.uniform(0, 120, (257, 2)) + [4.0e6, 2.2e6], r.integers(0, 2, 257).astype(np.int32)      # 257: a second workgroup of one point
    conf = confidences(257, 5)
    for S in (1, 12, 32):
        check_member(xy, group, conf, subset_masks(257, S, 6), 12.0, 10, S)
    one = member_subsets_gpu(xy, group, conf, np.ones(257, np.uint32), 12.0, 10, 1)
    assert torch.equal(one[0], member_gpu(xy, group, conf, 12.0, 10))                # S = 1, every bit set: aq_eval_member_conf_f64's bytes
    top = member_subsets_gpu(xy, group, conf, np.full(257, 1 << 31, np.uint32), 12.0, 10, 32)
    assert torch.equal(top[31], one[0]) and bool((top[:31] == NEG_INF).all())           # bit 31 alone
    det = fixture_data()["det"]
    assert det["conf"].shape[0] == 1095
    mask = subset_masks(1095, 12, 8)
    for eps in (10.0, 50.0, 150.0):
        check_member(det["xy"], det["year_id"], det["conf"], mask, eps, 10, 12)
    a = member_subsets_gpu(det["xy"], det["year_id"], det["conf"], mask, 50.0, 10, 12)
    b = member_subsets_gpu(det["xy"], det["year_id"], det["conf"], mask, 50.0, 10, 12)
    assert torch.equal(a, b)
    assert member_subsets_gpu(np.zeros((0, 2)), np.zeros(0), np.zeros(0), np.zeros(0, np.uint32), 10.0, 4, 3).shape == (3, 0, 4)


# ---- box_match_subsets ----

EDGE_K = np.array([[1.0, 0.0, 2.0, 1.0], [5.0, 4.0, 6.0, 5.0], [0.0, 0.0, 9.0, 9.0], [7.0, 7.0, 7.0, 7.0]])
EDGE_KG = np.array([0, 0, 1, 0], np.int32)
EDGE_Q = np.array([[0.0, 0.0, 1.0, 1.0],                   # touches key 0 along an edge
                   [2.0, 1.0, 3.0, 2.0],                   # touches key 0 at a corner
                   [5.0, 5.0, 5.0, 5.0],                   # a point on key 1's edge
                   [7.0, 7.0, 7.0, 7.0],                   # a point on a point
                   [3.0, 0.0, 4.0, 1.0],                   # nothing
                   [np.nextafter(2.0, 3.0), 0.0, 3.0, 1.0]])   # one ulp beside key 0


@pytest.mark.parametrize("S", [1, 12, 32])
def test_box_match_subsets_edges_corners_degenerate_boxes_and_masks(lib, S):
    top = np.uint32(1 << (S - 1))                           # bit 31 with S = 32
    pay = np.stack([np.array([[0.25, 1.0], [0.5, 2.0], [0.75, 3.0], [0.125, 4.0]]) + s for s in range(S)])
    full = np.full(6, (1 << S) - 1, np.uint32)
    hit, out = check_match(EDGE_Q, np.zeros(6, np.int32), full, EDGE_K, EDGE_KG, np.full(4, (1 << S) - 1, np.uint32), 2, S, pay)
    assert (hit == np.where([True, True, True, True, False, False], full, 0)).all()
    assert out[S - 1].tolist() == [[0.25 + S - 1, S], [0.25 + S - 1, S], [0.5 + S - 1, 1.0 + S], [0.125 + S - 1, 3.0 + S], [NEG_INF] * 2, [NEG_INF] * 2]
    # key 0 only in the top subset, query 1 only in the lowest: the corner match of query 1 counts in neither unless S = 1
    km = np.array([top, top | 1, top | 1, top | 1], np.uint32)
    qm = np.array([top | 1, 1, top | 1, top, top | 1, top | 1], np.uint32)
    hit, out = check_match(EDGE_Q, np.zeros(6, np.int32), qm, EDGE_K, EDGE_KG, km, 2, S, pay)
    assert hit.tolist() == ([1, 1, 1, 1, 0, 0] if S == 1 else [int(top), 0, int(top) | 1, int(top), 0, 0])
    hit, _ = check_match(EDGE_Q, np.ones(6, np.int32), qm, EDGE_K, EDGE_KG, km, 2, S)
    assert (hit == qm).all()
    # groups without keys (G = 4: groups 2 and 3), group ids out of range, one query, no keys, no queries
    hit, out = check_match(EDGE_Q, np.array([2, 3, -1, 4, 1 << 30, -(1 << 31)], np.int32), full, EDGE_K, EDGE_KG, km, 4, S, pay)
    assert not hit.any() and (out == NEG_INF).all()
    check_match(EDGE_Q[:1], np.zeros(1, np.int32), full[:1], EDGE_K, EDGE_KG, km, 2, S, pay)
    hit, out = check_match(EDGE_Q, np.zeros(6, np.int32), full, np.zeros((0, 4)), np.zeros(0, np.int32), np.zeros(0, np.uint32), 2, S, np.zeros((S, 0, 3)))
    assert not hit.any() and out.shape == (S, 6, 3) and (out == NEG_INF).all()
    assert match_subsets_gpu(np.zeros((0, 4)), np.zeros(0, np.int32), np.zeros(0, np.uint32), EDGE_K, EDGE_KG, km, 2, S, pay)[1].shape == (S, 0, 2)


@pytest.mark.parametrize("S", [1, 12, 32])
def test_box_match_subsets_long_runs_and_odd_query_counts(lib, S):
    """Group 0: 300 keys that all meet query 0 (the 64 lanes stride five times), the maximum of each payload column at another key of each
    subset; group 1: the query's x1 cuts the sorted run after 70 keys; group 2: keys left of the query; 7 queries (not a multiple of 4)."""
    r = np.random.default_rng(3)
    x0 = np.concatenate([r.uniform(0, 50, 300), np.arange(200) * 1.0, r.uniform(-500, -100, 130)])
    k = np.stack([x0, np.zeros(630), x0 + 10.0, np.full(630, 10.0)], 1)
    kg = np.repeat(np.array([0, 1, 2], np.int32), [300, 200, 130])
    km = subset_masks(630, S, 9)
    pay = r.permutation(S * 630 * 16).reshape(S, 630, 16).astype(np.float64)
    q = np.array([[10.0, 2.0, 60.0, 3.0], [-5.0, 2.0, 69.0, 3.0], [0.0, 2.0, 1.0, 3.0], [10.0, 2.0, 60.0, 3.0], [20.0, 0.0, 21.0, 1.0],
                  [10.0, 2.0, 60.0, 3.0], [-5.0, 20.0, 69.0, 30.0]])
    qg = np.array([0, 1, 2, 0, 0, 1, 1], np.int32)
    qm = np.array([(1 << S) - 1, (1 << S) - 1, (1 << S) - 1, 1 << (S - 1), 0, 1, (1 << S) - 1], np.uint32)
    perm = r.permutation(630)
    hit, out = check_match(q, qg, qm, k[perm], kg[perm], km[perm], 3, S, pay[:, perm])
    in_top = ((km[:300] >> np.uint32(S - 1)) & 1).astype(bool)
    assert np.array_equal(out[S - 1, 0], pay[S - 1, :300][in_top].max(0)) and hit[2] == 0 and hit[4] == 0 and hit[6] == 0
    assert hit[3] == 1 << (S - 1) and np.array_equal(out[S - 1, 3], out[S - 1, 0]) and (S == 1 or (out[:S - 1, 3] == NEG_INF).all())
    check_match(q, qg, qm, k[perm], kg[perm], km[perm], 3, S, pay[:, perm][:, :, :1])
    check_match(q, qg, qm, k[perm], kg[perm], km[perm], 3, S)
    h2, o2 = match_subsets_gpu(q, qg, qm, k[perm], kg[perm], km[perm], 3, S, pay[:, perm])
    assert np.array_equal(hit, h2) and np.array_equal(out, o2)


def test_box_match_subsets_of_the_fixture_respects_the_subsets(lib):
    data = fixture_data()
    det, lab = data["det"], data["lab"]
    dm, lm = subset_masks(1095, 12, 1), subset_masks(991, 12, 2)
    G = 2 * data["years"].shape[0]
    M = kfold.member_conf_subsets_numpy(det["xy"], det["year_id"], det["conf"], dm, 50.0, 10, 12)
    hit, _ = check_match(det["box"], det["group"], dm, lab["box"], lab["group"], lm, G, 12)
    check_match(lab["box"], lab["group"], lm, det["box"], det["group"], dm, G, 12, M)
    whole = evaluate.box_match_numpy(det["box"], det["group"], lab["box"], lab["group"])[0]
    assert ((hit != 0) <= whole).all() and (whole & (hit != dm)).any()      # a detection of a subset whose labels lie in others


# ---- one kernel source for both forms: all-ones masks give the plain entries' bytes ----

ALL = 0xFFFFFFFF


def lattice_points():
    """257 points (a full workgroup of 256 and one thread of the next) of a 0.5 m lattice, two groups, eps = 1.0: a point has up to 13
    neighbours, four of them at exactly eps, and the confidences take 7 values, so that equal confidences meet in every list."""
    i = np.arange(257)
    xy = np.stack([i % 17, i // 17], 1) * 0.5 + [4.0e6, 2.2e6]
    conf = np.array([0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9])[np.random.default_rng(12).integers(0, 7, 257)]
    return xy, (i >= 128).astype(np.int32), conf, 1.0


@pytest.mark.parametrize("K", [1, 3, 5, 16])                 # one per list size the launcher instantiates: 1, 4, 8, 16
def test_member_conf_with_all_ones_masks_is_the_plain_entrys_bytes(lib, K):
    xy, group, conf, eps = lattice_points()
    want = evaluate.member_conf_numpy(xy, group, conf, eps, K)
    assert np.unique(conf).size == 7 and np.isfinite(want[:, 0]).all() and (K < 14 or (want[:, 13:] == NEG_INF).all())
    plain = member_gpu(xy, group, conf, eps, K).cpu().numpy()
    assert plain.tobytes() == want.tobytes()
    for S in (1, 32):
        sub = member_subsets_gpu(xy, group, conf, np.full(257, ALL, np.uint32), eps, K, S).cpu().numpy()
        assert sub.shape == (S, 257, K)
        for s in range(S):
            assert sub[s].tobytes() == plain.tobytes(), s


@functools.lru_cache(None)
def join_case(N):
    """5 queries (a second workgroup with one busy wave) against a run of N keys of group 0 (group 1 has none), integer boxes, 3 payload
    columns.  Query 0 covers every key, 1 touches the key with the largest x0 -- the last of the sorted run -- at a corner, 2 touches the
    first key along an edge, 3 covers everything but is of group 1, 4 lies apart."""
    r = np.random.default_rng(7)
    x0, y0 = r.integers(0, 12, N), r.integers(0, 12, N)
    k = np.stack([x0, y0, x0 + r.integers(1, 4, N), y0 + r.integers(1, 4, N)], 1).astype(np.float64)
    if N:
        k[-1] = [14.0, 3.0, 16.0, 5.0]                      # alone at the largest x0
    last, first = (k[-1], k[0]) if N else (np.array([14.0, 3.0, 16.0, 5.0]), np.array([0.0, 0.0, 1.0, 1.0]))
    q = np.array([[0.0, 0.0, 20.0, 20.0], [last[2], last[3], last[2] + 1.0, last[3] + 1.0], [first[0] - 1.0, first[1], first[0], first[3]],
                  [0.0, 0.0, 20.0, 20.0], [30.0, 30.0, 31.0, 31.0]])
    qg = np.array([0, 0, 0, 1, 0], np.int32)
    return q, qg, k, np.zeros(N, np.int32), r.permutation(3 * N).reshape(N, 3).astype(np.float64)


@functools.lru_cache(None)
def join_reference(N):
    """box_match_numpy of join_case(N), and that the case holds what it is built for: no case but N = 0 is empty."""
    q, qg, k, kg, pay = join_case(N)
    hit, out = evaluate.box_match_numpy(q, qg, k, kg, pay)
    if N == 0:
        assert not hit.any() and (out == NEG_INF).all()
        return hit, out
    assert hit.tolist() == [True, True, True, False, False]
    w = np.minimum(q[1:3, None, 2], k[None, :, 2]) - np.maximum(q[1:3, None, 0], k[None, :, 0])
    h = np.minimum(q[1:3, None, 3], k[None, :, 3]) - np.maximum(q[1:3, None, 1], k[None, :, 1])
    meet = (w >= 0) & (h >= 0)
    assert (meet & (w * h == 0)).any(1).all()               # queries 1 and 2 each touch a key without overlapping it: a corner, an edge
    # query 1 meets the last key of the sorted run and no other: with N = 65 that is position 64, the second step of lane 0
    assert np.lexsort((k[:, 0], kg))[-1] == N - 1 and meet[0].nonzero()[0].tolist() == [N - 1] and np.array_equal(out[1], pay[N - 1])
    return hit, out


@pytest.mark.parametrize("N", [0, 63, 65])                   # no key; one short of the lanes' stride; one past it
def test_box_match_with_all_ones_masks_is_the_plain_entrys_bytes(lib, N):
    q, qg, k, kg, pay = join_case(N)
    want_hit, want_out = join_reference(N)
    hit, out = match_gpu(q, qg, k, kg, 2, pay)
    assert np.array_equal(hit, want_hit) and out.tobytes() == want_out.tobytes()
    for S in (1, 32):
        hitmask, outs = match_subsets_gpu(q, qg, np.full(5, ALL, np.uint32), k, kg, np.full(N, ALL, np.uint32), 2, S, np.tile(pay, (S, 1, 1)))
        assert np.array_equal(hitmask, np.where(hit, np.uint32(ALL >> (32 - S)), np.uint32(0)))
        assert outs.shape == (S, 5, 3)
        for s in range(S):
            assert outs[s].tobytes() == out.tobytes(), s


@pytest.mark.parametrize("N", [0, 63, 65])
def test_model_error_match_has_box_matchs_candidates(lib, N):
    from aquaculture_amd.engine import model_error_match
    q, qg, k, kg, _ = join_case(N)
    want_hit, _ = join_reference(N)
    match = model_error_match(dev(q, np.float64), dev(qg, np.int32), dev(np.ones(5), np.float64), dev(k.reshape(-1, 4), np.float64), dev(kg, np.int32),
                              dev(np.ones(N), np.float64), 2)[0].cpu().numpy()
    assert np.array_equal(match >= 0, want_hit) and np.array_equal(match_gpu(q, qg, k, kg, 2)[0], want_hit)


# ---- the poisoned allocator ----

def test_nothing_depends_on_unowned_bytes(lib, monkeypatch):
    xy, group, eps, _ = CASES["blobs_0"]
    n = xy.shape[0]
    conf, mask = confidences(n, 7), subset_masks(n, 12, 3)
    pay = np.stack([np.array([[0.25, 1.0], [0.5, 2.0], [0.75, 3.0], [0.125, 4.0]]) + s for s in range(12)])
    km = np.array([1 << 11, 3, 3, 1 << 11 | 1], np.uint32)
    qm = np.array([3, 1 << 11, 1, 1, 3, 0], np.uint32)
    outs = {}
    for byte in (0x00, 0xFF):
        with poisoned(monkeypatch, byte) as p:
            M = member_subsets_gpu(xy, group, conf, mask, eps, 10, 12)
            hit, out = match_subsets_gpu(EDGE_Q, np.zeros(6, np.int32), qm, EDGE_K, EDGE_KG, km, 2, 12, pay)
            hit0, _ = match_subsets_gpu(EDGE_Q, np.zeros(6, np.int32), qm, EDGE_K, EDGE_KG, km, 2, 12)
            torch.cuda.synchronize()
            outs[byte] = (M.cpu().numpy().copy(), hit.copy(), out.copy(), hit0.copy())
            p.check_guards()
            assert not p.passed_through, p.passed_through
    for a, b in zip(outs[0x00], outs[0xFF]):
        assert a.tobytes() == b.tobytes()                   # the same bytes under both fills: nothing read that the call did not write
    M, hit, out, hit0 = outs[0xFF]
    assert not np.isnan(M).any() and not np.isnan(out).any()                 # fully written: 0xFF is NaN in fp64
    assert np.array_equal(M, kfold.member_conf_subsets_numpy(xy, group, conf, mask, eps, 10, 12))
    want_hit, want_out = kfold.box_match_subsets_numpy(EDGE_Q, np.zeros(6, np.int32), qm, EDGE_K, EDGE_KG, km, 12, pay)
    assert np.array_equal(hit, want_hit) and np.array_equal(hit0, want_hit) and np.array_equal(out, want_out)


# ---- refusals ----

def test_bad_arguments_are_refused_and_nothing_is_launched(lib):
    from aquaculture_amd import engine
    xy, group, eps, _ = CASES["blobs_1"]
    n, K, S = xy.shape[0], 5, 3
    conf_h, mask_h = confidences(n, 2), subset_masks(n, S, 4)
    x, g, c = torch.from_numpy(xy).cuda(), torch.from_numpy(group).cuda(), torch.from_numpy(conf_h).cuda()
    m = torch.from_numpy(mask_h.astype(np.int32)).cuda()
    keys, perm = engine.facility_sort_keys(x, g, eps)
    need = int(lib.aq_eval_subsets_scratch_bytes(n, K, S))
    scratch = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")
    M = torch.full((S, n, K), -77.0, dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def call(keys_p=keys.data_ptr(), conf_p=c.data_ptr(), mask_p=m.data_ptr(), n_=n, eps_=eps, K_=K, S_=S, scratch_bytes=need, out_p=M.data_ptr(), xy_p=x.data_ptr()):
        return lib.aq_eval_member_conf_subsets_f64(keys_p, perm.data_ptr(), xy_p, g.data_ptr(), conf_p, mask_p, n_, eps_, K_, S_, scratch.data_ptr(),
                                                   scratch_bytes, out_p, stream)

    for kw, msg in (({"S_": 0}, "S = 0"), ({"S_": 33}, "S = 33"), ({"K_": 0}, "K = 0"), ({"K_": 17}, "K = 17"), ({"eps_": 0.0}, "eps"), ({"eps_": -1.0}, "eps"),
                    ({"eps_": float("nan")}, "eps"), ({"eps_": float("inf")}, "eps"), ({"keys_p": None}, "null pointer"), ({"conf_p": None}, "null pointer"),
                    ({"mask_p": None}, "null pointer"), ({"out_p": None}, "null pointer"), ({"n_": 1 << 31}, "2\\^31"), ({"n_": -1}, "2\\^31"),
                    ({"n_": 1 << 27, "K_": 16, "S_": 32}, "2\\^36"), ({"scratch_bytes": need - 1}, "scratch"), ({"xy_p": x.data_ptr() + 8}, "unaligned"),
                    ({"conf_p": c.data_ptr() + 4}, "unaligned"), ({"mask_p": m.data_ptr() + 2}, "unaligned")):
        assert call(**kw) == -1, kw
        assert re.search(msg, lib.aq_last_error().decode()), (kw, lib.aq_last_error())
        torch.cuda.synchronize()
        assert bool((M == -77.0).all()) and bool((scratch == 0x5A).all()), kw
    assert lib.aq_eval_member_conf_subsets_f64(None, None, None, None, None, None, 0, eps, K, S, None, 0, None, stream) == 0      # n = 0 does nothing
    with pytest.raises(ValueError, match="S = 33"):
        engine.eval_member_conf_subsets(x, g, c, m, eps, K, 33)
    with pytest.raises(ValueError, match="K = 17"):
        engine.eval_member_conf_subsets(x, g, c, m, eps, 17, S)
    with pytest.raises(ValueError, match="eps"):
        engine.eval_member_conf_subsets(x, g, c, m, 0.0, K, S)

    q = torch.tensor([[0.0, 0.0, 1.0, 1.0], [5.0, 5.0, 6.0, 6.0]], dtype=torch.float64, device="cuda")
    qg = torch.zeros(2, dtype=torch.int32, device="cuda")
    qm = torch.tensor([3, 3], dtype=torch.int32, device="cuda")
    kb = torch.tensor([[0.5, 0.5, 2.0, 2.0]], dtype=torch.float64, device="cuda")
    km = torch.tensor([2, 0], dtype=torch.int32, device="cuda")
    start = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    pay = torch.tensor([[[0.5, 0.25]], [[0.75, 0.125]]], dtype=torch.float64, device="cuda")
    hit = torch.full((2,), 0x77777777, dtype=torch.int32, device="cuda")
    out = torch.full((2, 2, 2), -77.0, dtype=torch.float64, device="cuda")

    def match(q_p=q.data_ptr(), qm_p=qm.data_ptr(), Q_=2, k_p=kb.data_ptr(), km_p=km.data_ptr(), N_=1, start_p=start.data_ptr(), G_=1, pay_p=pay.data_ptr(),
              K_=2, S_=2, hit_p=hit.data_ptr(), out_p=out.data_ptr()):
        return lib.aq_box_match_subsets_f64(q_p, qg.data_ptr(), qm_p, Q_, k_p, km_p, N_, start_p, G_, pay_p, K_, S_, hit_p, out_p, stream)

    for kw, msg in (({"S_": 0}, "S = 0"), ({"S_": 33}, "S = 33"), ({"K_": 17}, "K = 17"), ({"K_": -1}, "K = -1"), ({"Q_": 1 << 31}, "2\\^31"),
                    ({"N_": 1 << 31}, "2\\^31"), ({"Q_": -1}, "2\\^31"), ({"Q_": 1 << 27, "K_": 16, "S_": 32}, "2\\^36"), ({"G_": -1}, "groups"),
                    ({"q_p": None}, "null pointer"), ({"qm_p": None}, "null pointer"), ({"k_p": None}, "null pointer"), ({"km_p": None}, "null pointer"),
                    ({"start_p": None}, "null pointer"), ({"hit_p": None}, "null pointer"), ({"pay_p": None}, "null pointer"), ({"out_p": None}, "null pointer"),
                    ({"q_p": q.data_ptr() + 16}, "unaligned"), ({"k_p": kb.data_ptr() + 8}, "unaligned"), ({"out_p": out.data_ptr() + 4}, "unaligned"),
                    ({"qm_p": qm.data_ptr() + 2}, "unaligned"), ({"hit_p": hit.data_ptr() + 2}, "unaligned")):
        assert match(**kw) == -1, kw
        assert re.search(msg, lib.aq_last_error().decode()), (kw, lib.aq_last_error())
        torch.cuda.synchronize()
        assert bool((hit == 0x77777777).all()) and bool((out == -77.0).all()), kw
    assert lib.aq_box_match_subsets_f64(None, None, None, 0, None, None, 0, None, 0, None, 0, 1, None, None, stream) == 0        # Q = 0 does nothing
    with pytest.raises(ValueError, match="group ids"):
        engine.box_match_subsets(q, qg, qm, kb, torch.tensor([1], dtype=torch.int32, device="cuda"), km[:1], 1, 2)
    with pytest.raises(ValueError, match="S = 33"):
        engine.box_match_subsets(q, qg, qm, kb, torch.zeros(1, dtype=torch.int32, device="cuda"), km[:1], 1, 33)
    torch.cuda.synchronize()
    assert bool((M == -77.0).all()) and bool((scratch == 0x5A).all()) and bool((hit == 0x77777777).all()) and bool((out == -77.0).all())
    assert call() == 0 and match() == 0                     # and the same arguments, all valid, run
    torch.cuda.synchronize()
    assert torch.equal(M.cpu(), torch.from_numpy(kfold.member_conf_subsets_numpy(xy, group, conf_h, mask_h, eps, K, S)))
    assert hit.tolist() == [2, 0] and out.tolist() == [[[NEG_INF] * 2] * 2, [[0.75, 0.125], [NEG_INF] * 2]]


# ---- end to end ----

def same_kfold_files(got_dir, want_dir, device=True):
    for name in (kfold.RESULTS_FILE, kfold.IMAGES_FILE):
        assert open(os.path.join(got_dir, name)).read() == open(os.path.join(want_dir, name)).read(), name
    if device:
        assert open(os.path.join(got_dir, kfold.JSON_FILE)).read() == open(os.path.join(want_dir, kfold.JSON_FILE)).read()
    got, want = (json.load(open(os.path.join(d, kfold.JSON_FILE))) for d in (got_dir, want_dir))
    assert {k: v for k, v in got.items() if k != "device"} == {k: v for k, v in want.items() if k != "device"}
    return got


@pytest.mark.parametrize("N", [3, 5])
def test_kfold_files_are_the_host_paths_byte_for_byte(lib, tmp_path, N):
    """The device is recorded in kfold.json, so both runs are given one name for it; every other byte is the run's own."""
    names, rects, sites = kfold_inputs()
    kw = dict(names=names, rects=rects, sites=sites, conf_grid=SMALL_GRID[0], eps_grid=SMALL_GRID[1], min_grid=SMALL_GRID[2], op=(0.785, 50.0, 5), device="a device")
    times = {}
    s = evaluate.kfold(detection_table(), truth(), str(tmp_path / "gpu"), N, times=times, **kw)
    evaluate.kfold(detection_table(), truth(), str(tmp_path / "cpu"), N, cpu=True, **kw)
    got = same_kfold_files(str(tmp_path / "gpu"), str(tmp_path / "cpu"))
    assert got == s and times["kernel_ms"] > 0 and s["holdout"]["cage"]["n_label"] > 0
    assert torch.cuda.get_device_name() == json.load(open(_default_device(tmp_path)))["device"]


def _default_device(tmp_path):
    out = str(tmp_path / "named")
    evaluate.kfold(detection_table(), truth(), out, 2, conf_grid=SMALL_GRID[0][:1], eps_grid=SMALL_GRID[1][:1], min_grid=SMALL_GRID[2][:1], test_frac=0)
    return os.path.join(out, kfold.JSON_FILE)


def test_full_grid_phase_is_evaluate_grid_per_fold(lib):
    """The batched grid phase over the default 82 x 8 x 10 grid against the path the parent commit has: evaluate.grid on every fold's images."""
    from test_kfold import fixture_images
    data, images, names = fixture_images()
    split = kfold.split_images(images["bucket"], 3, 1, 0.1)
    w = kfold.subset_words(split, 3)
    tables = kfold.fold_grids(data, w[images["det_row"]], w[images["lab_row"]], 3, evaluate.DEFAULT_CONF, evaluate.DEFAULT_EPS, evaluate.DEFAULT_MIN)
    for f in range(3):
        fold_names = [n for n, s in zip(names, split) if s >= 0 and s != f]
        want = evaluate.grid(evaluate.inputs(detection_table(), truth(), images=fold_names))
        for c in evaluate.COLUMNS:
            assert np.array_equal(tables[f][c], want[c], equal_nan=True), (f, c)


def test_command_line_matches_the_host_restatement(lib, tmp_path):
    labels, csv_path = synthetic_run(tmp_path)
    truth_path = lattice_truth(tmp_path / "truth.geojson", csv_path)
    (bx0, _, _, by1), = geocode.load_wanted_bboxes(csv_path).values()
    lon, lat = geocode.mercator_to_lonlat(np.float64(bx0 + 100.0), np.float64(by1 - 100.0))      # in the scene's north-west tile: four tile columns meet its box
    (tmp_path / "sites.csv").write_text(f"id,lat,lon,num_cages\n1,{float(lat)!r},{float(lon)!r},10\n2,50.0,3.5,4\n")
    out = str(tmp_path / "gpu")
    args = ["--evaluate-kfold", "2", "--evaluate-known-sites", str(tmp_path / "sites.csv"), "--evaluate-kfold-seed", "3"]
    r = subprocess.run([sys.executable, "-m", "aquaculture_amd.evaluate", "--labels", labels, "--geocode-bboxes", csv_path, "--truth", truth_path,
                        "--evaluate-out", out, "--facilities-conf", "0.5", "--facilities-eps", "10", "--facilities-min-cages", "5", *GRID_ARGS, *args],
                       cwd=ROOT, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "2-fold cross-validation over 13 images (2 set aside)" in r.stdout, r.stdout
    table = geocode.geocode_label_dir(labels, csv_path)
    want = str(tmp_path / "cpu")
    evaluate.kfold_from_options(table, truth_path, want, GRIDS, (0.5, 10.0, 5), None, None, 2, None, str(tmp_path / "sites.csv"), 3, 0.1, csv_path, cpu=True)
    s = same_kfold_files(out, want, device=False)
    assert s["device"] == torch.cuda.get_device_name() and s["parameters"]["known_sites"] == 2 and s["n_images"] == 15
    counts = {b["bucket"]: b["images"] for b in s["strata"]}
    assert counts["(0.8, 1.0]"] == 3 and counts[kfold.NO_DET_IN] > 0 and counts[kfold.NO_DET_IN] + counts[kfold.NO_DET_OUT] == 12
    assert sorted(os.listdir(out)) == sorted([evaluate.CSV_FILE, evaluate.JSON_FILE, *evaluate.KFOLD_FILES])


def test_detect_py_cross_validates_its_own_sweep(lib, tmp_path):
    """An engine sweep over eight synthetic 640-px tiles, geocoded and cross-validated in the same run: the image table holds every image of
    the sweep, and the three files equal what the host path makes of the run's label files."""
    from PIL import Image
    from aquaculture_amd import checkpoint, tiles
    (tmp_path / "jpegs").mkdir()
    stems = []
    for k, i in enumerate((0, 3, 19, 20, 1, 2, 4, 5)):
        stems.append(f"ORTHOIMAGERY.ORTHOPHOTOS{2015 - k % 2}_3_{1024 * (k % 4)}_{1024 * (k // 4)}")
        Image.fromarray(tiles.synthetic_tile(i, 640)).save(tmp_path / "jpegs" / (stems[-1] + ".jpeg"), quality=95)
    checkpoint.write_synthetic_checkpoint(str(tmp_path / "synth.pt"), "yolov5m", 5)
    _, csv_path = synthetic_run(tmp_path)
    truth_path = lattice_truth(tmp_path / "truth.geojson", csv_path)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "yolov5", "detect.py"), "--weights", str(tmp_path / "synth.pt"), "--source",
                        str(tmp_path / "jpegs"), "--save-txt", "--save-conf", "--nosave", "--project", str(tmp_path / "runs"), "--name", "kf",
                        "--batch-size", "4", "--geocode-bboxes", csv_path, "--facilities-conf", "0.25", "--facilities-eps", "25",
                        "--facilities-min-cages", "4", "--evaluate", truth_path, *GRID_ARGS, "--evaluate-kfold", "2", "--evaluate-kfold-test", "0"],
                       capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    run = tmp_path / "runs" / "kf"
    assert "2-fold cross-validation over 8 images (0 set aside)" in r.stdout + r.stderr
    table = geocode.geocode_label_dir(str(run / "labels"), csv_path)
    want = str(tmp_path / "want")
    evaluate.kfold_from_options(table, truth_path, want, GRIDS, (0.25, 25.0, 4), None, None, 2, None, None, 1, 0.0, csv_path, names=sorted(stems), cpu=True)
    s = same_kfold_files(str(run), want, device=False)
    assert s["n_images"] == 8 and s["holdout"] is None and kfold.read_images_csv(str(run / kfold.IMAGES_FILE))["image"] == sorted(stems)
