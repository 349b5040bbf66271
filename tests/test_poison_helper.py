"""The poisoned allocator of tests/poison.py on the CPU: the same code path the GPU tests use, with CPU allocations intercepted under
the helper's ``cpu`` flag (a CUDA device and pinned memory both need a GPU)."""
import pytest
import torch

from poison import GUARD_BYTE, Poison, _is_cuda, poisoned


@pytest.mark.parametrize("byte", [0x00, 0xFF])
def test_fill_is_applied(monkeypatch, byte):
    with poisoned(monkeypatch, byte, guard=64, cpu=True) as p:
        a = torch.empty((3, 5), dtype=torch.float32)
        b = torch.empty(7, dtype=torch.bfloat16, device="cpu")
        c = torch.empty(2, 3, 4, dtype=torch.int32)
        d = torch.empty_like(a, dtype=torch.float64)
        e = torch.empty(0, dtype=torch.uint8)
        assert a.shape == (3, 5) and b.shape == (7,) and c.shape == (2, 3, 4) and d.shape == (3, 5) and d.dtype == torch.float64 and e.numel() == 0
        for t in (a, b, c, d):
            assert t.is_contiguous() and t.storage_offset() == 0
            assert (t.reshape(-1).view(torch.uint8) == byte).all()
        if byte == 0xFF:
            assert a.isnan().all() and b.isnan().all() and d.isnan().all() and (c == -1).all()
        else:
            assert (a == 0).all() and (c == 0).all()
        assert p.intercepted == 5 and [x[1] for x in p.allocations] == [(3, 5), (7,), (2, 3, 4), (3, 5), (0,)]
        # the guard follows the tensor in the same storage and holds another byte
        raw = a.as_strided((15 + 64,), (1,)).view(torch.uint8)
        assert (raw[60:] == GUARD_BYTE).all() and GUARD_BYTE != byte
        p.check_guards()


def test_alignment_is_that_of_an_ordinary_allocation(monkeypatch):
    plain = torch.empty(1000, dtype=torch.float32)
    with poisoned(monkeypatch, 0xFF, cpu=True):
        t = torch.empty(1000, dtype=torch.float32)
        assert t.data_ptr() % 64 == plain.data_ptr() % 64 == 0 and t.storage_offset() == 0


def test_pass_through_calls_are_untouched(monkeypatch):
    real = torch.empty
    with poisoned(monkeypatch, 0xFF, guard=64) as p:              # no cpu flag: a CPU allocation is none of the helper's business
        a = torch.empty((4, 4), dtype=torch.float32)
        b = torch.empty_like(a)
        assert a.untyped_storage().nbytes() == 64 and b.untyped_storage().nbytes() == 64      # no guard behind them
        assert p.intercepted == 0 and not p.allocations
    with poisoned(monkeypatch, 0xFF, guard=64, cpu=True) as p:    # with it: forms the helper does not model still pass through
        o = torch.zeros(4)
        assert torch.empty(4, out=o) is o
        assert torch.empty((2, 3, 4, 5), memory_format=torch.channels_last).untyped_storage().nbytes() == 120 * 4
        assert p.intercepted == 0
        assert torch.zeros(3).tolist() == [0, 0, 0] and torch.full((2,), 7.0).tolist() == [7, 7]
    assert torch.empty is real


def test_check_guards_catches_a_write_one_past_the_end(monkeypatch):
    with poisoned(monkeypatch, 0x00, guard=16, cpu=True) as p:
        torch.empty(3, dtype=torch.int32)
        t = torch.empty((2, 5), dtype=torch.float32)
        torch.empty((4,), dtype=torch.uint8)
        p.check_guards()
        t.as_strided((11,), (1,))[10] = 1.0                        # element 10 of 10: the first of the guard
        with pytest.raises(AssertionError, match=r"allocation #1 \(shape \(2, 5\), torch\.float32\).*element 10 of 10"):
            p.check_guards()


def test_torch_empty_is_restored_on_exit(monkeypatch):
    real, real_like = torch.empty, torch.empty_like
    with poisoned(monkeypatch, 0xFF, cpu=True):
        assert torch.empty is not real and torch.empty_like is not real_like
    assert torch.empty is real and torch.empty_like is real_like
    with pytest.raises(RuntimeError):
        with poisoned(monkeypatch, 0xFF, cpu=True):
            raise RuntimeError("leaving through an exception")
    assert torch.empty is real and torch.empty_like is real_like
    assert torch.empty(5).untyped_storage().nbytes() == 20


def test_routing_of_cuda_and_pinned_requests():
    """What the GPU tests rely on, without a GPU: which (device, pin_memory) requests are intercepted."""
    assert _is_cuda("cuda") and _is_cuda("cuda:0") and _is_cuda(torch.device("cuda", 1)) and _is_cuda(0) and _is_cuda(3)
    assert not _is_cuda(None) and not _is_cuda("cpu") and not _is_cuda(torch.device("cpu"))
    p = Poison(0xFF, 16, cpu=False)
    assert p._wants("cuda:0", None) and p._wants(0, False) and p._wants(None, True) and p._wants("cpu", True)
    assert not p._wants(None, None) and not p._wants("cpu", False) and not p._wants(torch.device("cpu"), None)
    q = Poison(0xFF, 16, cpu=True)
    assert q._wants(None, None) and q._wants("cpu", False) and q._wants("cuda", None)


def test_unmodelled_forms_are_recorded_not_silently_skipped(monkeypatch):
    with poisoned(monkeypatch, 0xFF, guard=16, cpu=True) as p:
        a = torch.empty(size=(2, 3), dtype=torch.float32)                      # the keyword form is modelled
        assert a.isnan().all() and p.intercepted == 1 and not p.passed_through
        torch.empty_like(torch.zeros(4, 6).t())                                # non-contiguous
        torch.empty_strided((2, 3), (3, 1))
        a.new_empty((5,))
        torch.empty((2, 3, 4, 5), memory_format=torch.channels_last)
        assert len(p.passed_through) == 4 and p.intercepted == 1
        assert "empty_like" in p.passed_through[0] and "empty_strided" in p.passed_through[1] and "new_empty" in p.passed_through[2]
        held = len(p.allocations)
    assert held == 1 and not p.allocations                                     # released with the block
    with poisoned(monkeypatch, 0xFF, guard=16) as p:                           # CPU requests outside the helper's business: not recorded
        torch.empty_strided((2, 3), (3, 1))
        torch.zeros(3).new_empty((5,))
        assert not p.passed_through
