"""tests/silu_range.py's bound is satisfiable by the bf16-mode instruction sequence itself, and refuses three plausible faults (CPU only).

The emulation follows the kernels' epilogue operation by operation in fp32:

    t = fl(z * fl(-1.44269504))     e = exp2(t) rounded to fp32     d = fl(1 + e)     r = fl(1 / d)     y = bf16_rne(fl(z * r))

with every result below 2^-126 flushed to zero (v_exp_f32 and v_rcp_f32 do not produce denormals) and with exp2 and the reciprocal each
pushed one ulp down, left alone, or pushed one ulp up -- nine combinations, the hardware's documented 1-ulp accuracy either way.
"""
import pytest
import torch

from silu_range import Z_GRID, grid_bias, grid_rotations, silu_tol

TINY = 2.0 ** -126


def flush(v):
    return torch.where(v.abs() < TINY, torch.zeros_like(v) * v.sign(), v)


def push(v, k):
    """v moved k ulps away from (k > 0) or towards (k < 0) zero; zeros and infinities stay."""
    if k == 0:
        return v
    moved = torch.nextafter(v, torch.full_like(v, float("inf") if k > 0 else 0.0))
    return torch.where((v == 0) | torch.isinf(v), v, moved)


def exp2_f32(t, k=0):
    return flush(push(torch.exp2(t.double()).float(), k))


def rcp_f32(d, k=0):
    return flush(push((1.0 / d.double()).float(), k))


def silu_bf16_mode(z, ke=0, kr=0):
    z = z.float()
    t = z * torch.tensor(-1.44269504, dtype=torch.float32)
    r = rcp_f32(1.0 + exp2_f32(t, ke), kr)
    return flush(z * r).bfloat16().float()


def silu_clamped(z):                            # valid on a clamped range only
    return silu_bf16_mode(z.float().clamp(-20.0, 20.0))


def silu_bf16_sigmoid(z):                       # the sigmoid carried in bf16, the product rounded again
    z = z.float()
    q = lambda v: v.bfloat16().float()
    e = q(exp2_f32(q(z * torch.tensor(-1.44269504, dtype=torch.float32))))
    r = q(rcp_f32(q(1.0 + e)))
    return flush(z * r).bfloat16().float()


def silu_unsaturated(z):                        # sigmoid as e^z * rcp(1 + e^z): the exp must stay finite for it, and does not: inf * 0
    z = z.float()
    e = exp2_f32(z * torch.tensor(1.44269504, dtype=torch.float32))
    return flush(z * (e * rcp_f32(1.0 + e))).bfloat16().float()


def test_the_grid_reaches_every_store_position():
    """After grid_rotations(cout) every value has sat in every position of an 8-channel store group, so in both lanes of a packed pair;
    the grid holds the values the kernels must see; a permutation moves values, it does not change them."""
    n = len(Z_GRID)
    for cout in (16, 32, 48, 64, 96, 192, 384):
        seen = {((c + r) % n, c % 8) for r in grid_rotations(cout) for c in range(cout)}
        assert seen == {(v, p) for v in range(n) for p in range(8)}, cout
        assert {(v, p % 2) for v, p in seen} == {(v, lane) for v in range(n) for lane in range(2)}
    assert len(grid_rotations(384)) == 1 and len(grid_rotations(16)) <= n
    must = [0.0, -1.2784645, 1, -1, 5, -5, 10, -10, 17, -17, 30, -30, 60, -60, -80, -87, -87.5, -88, -88.5, -88.72, -88.73, -89, -100, -104,
            88, 89, 100, 1000]
    assert set(must) <= set(Z_GRID) and any(str(v) == "-0.0" for v in Z_GRID)
    perm = [(5 * c + 3) % 48 for c in range(48)]
    assert torch.equal(grid_bias(48, 2, perm)[perm], grid_bias(48, 2))


def sweep():
    dense = torch.linspace(-110.0, 110.0, 1_200_001, dtype=torch.float64).float()
    return torch.cat([dense, torch.tensor(Z_GRID, dtype=torch.float32), torch.tensor([3e38, -3e38], dtype=torch.float32)])


def violations(got, z):
    ref, tol = silu_tol(z.double(), z.double().abs())              # a bias alone: A = |b| = |z|
    return ~((got.double() - ref).abs() <= tol)


@pytest.mark.parametrize("ke", [-1, 0, 1])
@pytest.mark.parametrize("kr", [-1, 0, 1])
def test_the_kernels_sequence_keeps_the_bound(ke, kr):
    z = sweep()
    assert z.numel() >= 10 ** 6
    got = silu_bf16_mode(z, ke, kr)
    assert not torch.isnan(got).any()
    bad = violations(got, z)
    assert not bad.any(), (int(bad.sum()), z[bad][:4].tolist(), got[bad][:4].tolist())


def test_the_tail_is_checked_relatively():
    """At z = -30 the bound admits about one bf16 rounding of -2.8e-12, not an absolute floor."""
    z = torch.tensor([-30.0], dtype=torch.float64)
    ref, tol = silu_tol(z, z.abs())
    assert abs(float(ref) + 2.8073e-12) < 1e-15 and float(tol) < 2.0 ** -7 * abs(float(ref))


@pytest.mark.parametrize("wrong", [silu_clamped, silu_bf16_sigmoid, silu_unsaturated])
def test_a_wrong_epilogue_violates_the_bound_on_the_grid(wrong):
    z = torch.tensor(Z_GRID, dtype=torch.float32)
    bad = violations(wrong(z), z)
    assert bad.any(), wrong.__name__
    assert not violations(silu_bf16_mode(z), z).any()
