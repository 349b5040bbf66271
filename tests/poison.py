"""A poisoned ``torch.empty`` for tests: nothing a kernel computes may depend on bytes it was never given.

``poisoned(monkeypatch, byte)`` replaces ``torch.empty`` and ``torch.empty_like`` inside a ``with`` block.  Every device (or pinned)
allocation made through them comes back filled with ``byte`` -- 0xFF reads as NaN in bf16, fp16, fp32, fp64 and e4m3 and as -1 in every
integer type -- and is followed by a guard of ``guard`` more elements holding another byte, which ``check_guards()`` verifies.  The
tensor handed out starts where an ordinary allocation of the caching allocator starts, so pointer alignment is what production sees.

``torch.empty_strided`` and ``Tensor.new_empty`` are wrapped too, but only to note device requests made through them
(``passed_through``): they are not poisoned.  The helper changes those four attributes of ``torch`` and nothing else: no environment
variable, no allocator setting, no start-up hook.  It is imported by tests (``from poison import poisoned``); it is not a conftest and defines no fixture.
"""
import contextlib
from typing import List, Tuple

import torch

GUARD_BYTE = 0xA5


def _size_of(args) -> Tuple[int, ...]:
    if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
        return tuple(int(s) for s in args[0])
    return tuple(int(s) for s in args)


def _numel(size) -> int:
    n = 1
    for s in size:
        n *= s
    return n


def _is_cuda(device) -> bool:
    if device is None:
        return False
    if isinstance(device, int):                      # a bare index means a CUDA device
        return True
    return torch.device(device).type == "cuda"


class Poison:
    """What ``poisoned`` yields: the allocations it handed out and the check of their guards."""

    def __init__(self, byte: int, guard: int, cpu: bool):
        assert 0 <= byte <= 0xFF and guard >= 1
        self.byte, self.guard, self.cpu = byte, guard, cpu
        self.guard_byte = GUARD_BYTE if byte != GUARD_BYTE else GUARD_BYTE ^ 0xFF
        self.allocations: List[Tuple[int, Tuple[int, ...], torch.dtype, torch.Tensor, int]] = []   # order, shape, dtype, flat, numel
        self.intercepted = 0
        self.passed_through: List[str] = []           # CUDA / pinned requests in a form the helper does not model: NOT poisoned
        self._empty = torch.empty
        self._empty_like = torch.empty_like
        self._empty_strided = torch.empty_strided
        self._new_empty = torch.Tensor.new_empty

    # ---- the replacements ----
    def _wants(self, device, pin_memory) -> bool:
        return bool(pin_memory) or _is_cuda(device) or (self.cpu and (device is None or torch.device(device).type == "cpu"))

    def _allocate(self, size, dtype, device, pin_memory) -> torch.Tensor:
        n = _numel(size)
        kw = {"dtype": dtype}
        if device is not None:
            kw["device"] = device
        if pin_memory:
            kw["pin_memory"] = True
        flat = self._empty(n + self.guard, **kw)
        raw = flat.view(torch.uint8)
        eb = flat.element_size()
        raw[:n * eb].fill_(self.byte)
        raw[n * eb:].fill_(self.guard_byte)
        order = self.intercepted
        self.intercepted += 1
        self.allocations.append((order, tuple(size), flat.dtype, flat, n))     # kept alive until the block ends: check_guards reads them
        return flat[:n].view(size)

    def _pass(self, what, device, pin_memory) -> None:
        if self._wants(device, pin_memory):
            self.passed_through.append(what)

    def empty(self, *args, **kw):
        kw = dict(kw)
        if "size" in kw and not args:
            args = (kw.pop("size"),)
        plain = set(kw) <= {"dtype", "device", "pin_memory", "requires_grad", "layout", "memory_format"}
        if (not plain or kw.get("requires_grad") or kw.get("layout", torch.strided) is not torch.strided
                or kw.get("memory_format", torch.contiguous_format) not in (torch.contiguous_format, torch.preserve_format)):
            self._pass(f"torch.empty({args}, {kw})", kw.get("device"), kw.get("pin_memory"))
            return self._empty(*args, **kw)
        if not self._wants(kw.get("device"), kw.get("pin_memory")):
            return self._empty(*args, **kw)
        return self._allocate(_size_of(args), kw.get("dtype") or torch.get_default_dtype(), kw.get("device"), kw.get("pin_memory"))

    def empty_like(self, t, **kw):
        device = kw.get("device", t.device)
        plain = set(kw) <= {"dtype", "device", "pin_memory"}
        if not plain or not t.is_contiguous() or t.layout is not torch.strided:
            self._pass(f"torch.empty_like(tensor of shape {tuple(t.shape)}, strides {t.stride()}, {kw})", device, kw.get("pin_memory"))
            return self._empty_like(t, **kw)
        if not self._wants(device, kw.get("pin_memory")):
            return self._empty_like(t, **kw)
        return self._allocate(tuple(t.shape), kw.get("dtype") or t.dtype, device, kw.get("pin_memory"))

    def empty_strided(self, *args, **kw):                    # not poisoned, only noted
        self._pass(f"torch.empty_strided({args}, {kw})", kw.get("device"), kw.get("pin_memory"))
        return self._empty_strided(*args, **kw)

    def new_empty(self, t, *args, **kw):                     # not poisoned, only noted
        self._pass(f"Tensor.new_empty({args}, {kw})", kw.get("device", t.device), kw.get("pin_memory"))
        return self._new_empty(t, *args, **kw)

    # ---- the check ----
    def check_guards(self) -> None:
        """Every guard still holds its byte; a damaged one is named by the allocation's requested shape, dtype and order."""
        for order, shape, dtype, flat, n in self.allocations:
            g = flat.view(torch.uint8)[n * flat.element_size():]
            if not bool((g != self.guard_byte).any()):
                continue
            at = int((g != self.guard_byte).nonzero()[0])
            raise AssertionError(f"allocation #{order} (shape {shape}, {dtype}) was written past its end: guard byte {at} "
                                 f"(element {n + at // flat.element_size()} of {n}) holds 0x{int(g[at]):02X}")


@contextlib.contextmanager
def poisoned(monkeypatch, byte: int, guard: int = 4096, cpu: bool = False):
    """Inside the block ``torch.empty`` / ``torch.empty_like`` calls that ask for a CUDA device or pinned memory return memory filled
    with ``byte``, followed by ``guard`` guard elements; every other call passes through untouched.  ``cpu=True`` (the helper's own CPU
    test) intercepts CPU allocations the same way.  Yields the ``Poison`` whose ``check_guards()`` the test calls before the block ends;
    ``passed_through`` lists the CUDA / pinned requests made in a form the helper does not poison (``torch.empty_strided``,
    ``Tensor.new_empty``, a non-contiguous ``empty_like``, unmodelled keywords), so that a test can assert there were none."""
    p = Poison(byte, guard, cpu)
    try:
        with monkeypatch.context() as m:
            m.setattr(torch, "empty", p.empty)
            m.setattr(torch, "empty_like", p.empty_like)
            m.setattr(torch, "empty_strided", p.empty_strided)
            m.setattr(torch.Tensor, "new_empty", lambda t, *a, **k: p.new_empty(t, *a, **k))
            yield p
    finally:
        p.allocations.clear()                        # the remembered tensors are released with the block
