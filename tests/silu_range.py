"""The activation range every fused bias + SiLU epilogue must survive, and the bound a correct one keeps -- test infrastructure (a plain
module: imported by tests/test_silu_range.py and tests/test_gpu_activation_range.py; no GPU, not a conftest, not collected).

Every convolution kernel carries its own copy of   y = z * rcp(1 + exp2(-log2(e) * z))   (bf16 mode, raw v_exp_f32 / v_rcp_f32) or of
z / (1 + expf(-z)) (fp32 mode).  The parity tests feed them randn inputs, He weights and biases of a few tenths, so z stays inside +-6; a
trained, BN-folded layer reaches many tens on both sides.  Z_GRID is laid over the output channels as the bias (grid_bias), the
convolution part keeps the usual data, so z = grid[c] + conv(x, w) sweeps the whole range in one small launch.

The bound (silu_tol), all quantities in float64, from the kernel's own operands (x and w already rounded to the storage type):

    z   = conv(x, w) + b                      y = z * sigmoid(z)            ref = y (+ res)
    s'  = sigmoid(z) * (1 + z * (1 - sigmoid(z)))                           A   = sum |x| |w| + |b|
    dz  = 2^-16 * A   (+ F, below)
    tol = 2^-8 |ref|  +  prop(dz)  +  2^-15 |y|  +  2^-16 |res|  +  2^-107
    prop(dz) = min( |s'| dz + dz^2 / 2 ,  max over |d| <= dz of |SiLU(z + d) - SiLU(z)| )

  2^-8 |ref|    one round-to-nearest-even to bf16 (8 significant bits: half an ulp is at most 2^-9 of the binade's top, 2^-8 of its bottom).
  dz            what the pre-activation can be off by: products of bf16 numbers are exact in fp32, the sum is taken in fp32 in k-steps of 32
                channels, K up to 1536.  Every term and every partial sum is rounded a bounded number of times, so the true error is of
                the order 2^-24 (A + sum_k |S_k|) (tests/cu_cases.py f8out_check works that model out); 2^-16 A is far above it and still
                256 times below one bf16 ulp of a value of size A.
  prop(dz)      how an error dz in z moves y.  Taylor: |s'| dz + dz^2 / 2, since |SiLU''| <= 1/2 everywhere.  On the negative tail that
                global second-order term dwarfs the value (z = -30, A = 35: dz^2 / 2 = 1.4e-7 against y = -2.8e-12), so the exact
                statement is taken where it is smaller: SiLU has one minimum, at ZMIN, hence over [z - dz, z + dz] the largest
                |SiLU(z + d) - SiLU(z)| is at an end of the interval or at ZMIN if the interval holds it.  Both are bounds on the same
                quantity, so is their minimum; it is never wider than the Taylor form, and it keeps the check RELATIVE on the tail: a
                kernel must give about -2.8e-12 at z = -30, not "anything below 1e-3".
  2^-15 |y|     the exp argument t = fl(z * fl(-log2 e)) is rounded once and the constant is off by 2^-26: exp2(t) is off by a factor
                |t| ln 2 * 1.25 * 2^-24 = 1.25 |z| 2^-24 <= 2^-16 for |z| <= 104 (beyond, exp2 has overflowed and y is an exact zero),
                which is y's relative error where sigmoid(z) ~ exp(z).  One ulp (2^-23) each for v_exp_f32, the add, v_rcp_f32 and the
                multiply fit in the other 2^-16.
  2^-16 |res|   the shortcut is added in fp32 before the one rounding to bf16; kept for the in-kernel conversions of res.
  2^-107        v_rcp_f32 flushes a denormal result: for 1 + exp2(t) in (2^126, 2^128), z in (-88.73, -87.34), the kernel's y is an exact
                zero where the true |y| = |z| exp(z) < 89 * 2^-126 < 2^-119; and beyond -88.73 exp2 is +inf, rcp gives 0, y = -0.  2^-107
                covers both with room (true |y| < 2^-109 for every z < -80.5).

fp32-mode kernels (IEEE divide, expf) use the same form with 2^-20 in place of both 2^-8 and 2^-15, dz = 2^-20 A (the suite's 2e-5 grade)
and a floor of 2^-120: expf overflows at z = -88.72 where the true |y| < 2^-120.

Without the activation (act=False) y = z, s' = 1 and there is no exp: tol = u |ref| + dz + 2^-16 |res| + floor.

Two-stage form (the fused two-stage kernels: t = bf16(SiLU(z1)) never leaves the CU, z2 = conv(t, w2) + b2).  The reference keeps t in
float64, UNROUNDED.  The kernel rounds its own fp32 t to bf16, to one of the two codes that neighbour the exact value: |dt_j| <= 2^-8 |t_j|.
So dz2 gains  F = 2^-8 sum_j |w2_j| |t_j|,  passed as `extra_dz`.  The same term covers an input that the kernel itself rounds to bf16
from an fp32 value it computed (the scaled stem's interpolated pixels).
"""
import math

import torch

ZMIN = -1.2784645427610738                    # SiLU's minimum: 1 + z (1 - sigmoid(z)) = 0
Z_GRID = (0.0, -0.0, -1.2784645, 1.0, -1.0, 5.0, -5.0, 10.0, -10.0, 17.0, -17.0, 30.0, -30.0, 60.0, -60.0,
          -80.0, -87.0, -87.5, -88.0, -88.5, -88.72, -88.73, -89.0, -100.0, -104.0, 88.0, 89.0, 100.0, 1000.0)
assert len(Z_GRID) == 29                      # odd and prime: coprime to every store-group and packed-pair width
GROUP = 8                                     # channels per 16-byte bf16 store; a packed pair is two neighbouring positions of it

MODES = {
    # output rounding, exp-argument / transcendental term, accumulation unit, floor
    "bf16": (2.0 ** -8, 2.0 ** -15, 2.0 ** -16, 2.0 ** -107),
    "fp32": (2.0 ** -20, 2.0 ** -20, 2.0 ** -20, 2.0 ** -120),
}


def grid_bias(cout, rot=0, perm=None):
    """fp32 bias [cout]: channel c holds Z_GRID[(c + rot) % 29]; `perm` (a permutation of range(cout)) moves channel c's value to
    channel perm[c]."""
    b = torch.tensor([Z_GRID[(c + rot) % len(Z_GRID)] for c in range(cout)], dtype=torch.float32)
    if perm is not None:
        out = torch.empty_like(b)
        out[torch.as_tensor(perm, dtype=torch.long)] = b
        b = out
    return b


def grid_rotations(cout):
    """The fewest rotations (greedy) after which every Z_GRID value has sat in every position of an 8-channel store group -- hence in both
    lanes of a packed pair -- of a cout-channel output.  One rotation where cout >= 232, all 29 for a 16-channel layer."""
    n = len(Z_GRID)
    need = {(v, p) for v in range(n) for p in range(min(GROUP, cout))}
    cover = {r: {((c + r) % n, c % GROUP) for c in range(cout)} for r in range(n)}
    rots = []
    while need:
        r = max(cover, key=lambda k: (len(cover[k] & need), -k))
        assert cover[r] & need
        rots.append(r)
        need -= cover[r]
    return rots


def silu64(z):
    return z * torch.sigmoid(z)


def silu_tol(z64, A, res=None, mode="bf16", act=True, extra_dz=None):
    """(ref, tol) per element, float64: the module docstring's bound.  z64: the pre-activation; A: sum |x| |w| + |b|; res: the shortcut
    added after the activation; extra_dz: the two-stage F."""
    u_out, u_arg, u_acc, floor = MODES[mode]
    z = z64.double()
    dz = u_acc * A.double()
    if extra_dz is not None:
        dz = dz + extra_dz.double()
    if act:
        s = torch.sigmoid(z)
        y = z * s
        taylor = (s * (1 + z * (1 - s))).abs() * dz + dz * dz / 2
        exact = torch.maximum((silu64(z + dz) - y).abs(), (silu64(z - dz) - y).abs())
        holds_min = (z - dz <= ZMIN) & (ZMIN <= z + dz)
        exact = torch.where(holds_min, torch.maximum(exact, y - ZMIN * torch.sigmoid(torch.tensor(ZMIN, dtype=torch.float64))), exact)
        prop = torch.minimum(taylor, exact) + u_arg * y.abs()
    else:
        y, prop = z, dz
    ref = y if res is None else y + res.double()
    tol = u_out * ref.abs() + prop + floor
    if res is not None:
        tol = tol + 2.0 ** -16 * res.double().abs()
    return ref, tol


WORST = {}                                    # family -> largest err / tol seen in this process (recorded, never asserted)


class RangeCheck:
    """One test's comparator: `add` one launch's output, `finish` asserts that the launches together spanned the range."""

    def __init__(self, family):
        self.family = family
        self.worst = 0.0
        self.zmin, self.zmax = math.inf, -math.inf
        self.near = torch.full((len(Z_GRID),), math.inf, dtype=torch.float64)
        self.grid = torch.tensor(Z_GRID, dtype=torch.float64)

    def span(self, z):
        """Record the pre-activations one launch's epilogue saw."""
        zf = z.double().reshape(-1)
        self.zmin, self.zmax = min(self.zmin, float(zf.min())), max(self.zmax, float(zf.max()))
        for i in range(0, zf.numel(), 1 << 18):
            self.near = torch.minimum(self.near, (zf[i:i + (1 << 18), None] - self.grid[None]).abs().amin(0))

    def add(self, got, z, ref, tol, what=""):
        got = got.detach().double().cpu()
        assert got.shape == ref.shape, (what, got.shape, ref.shape)
        assert bool(torch.isfinite(got).all()), f"{self.family} {what}: {int((~torch.isfinite(got)).sum())} values are not finite"
        err = (got - ref).abs()
        ratio = err / tol
        bad = ~(err <= tol)
        if bool(bad.any()):
            flat = torch.where(bad, ratio, torch.zeros_like(ratio)).reshape(-1)
            lines = [f"  z {float(z.reshape(-1)[i]):.9g}  got {float(got.reshape(-1)[i]):.9g}  ref {float(ref.reshape(-1)[i]):.9g}  "
                     f"tol {float(tol.reshape(-1)[i]):.3g}  (channel {int(i) % got.shape[-1]})" for i in torch.topk(flat, min(4, flat.numel())).indices]
            raise AssertionError(f"{self.family} {what}: {int(bad.sum())} of {bad.numel()} values outside the bound; the worst:\n" + "\n".join(lines))
        self.worst = max(self.worst, float(ratio.max()))
        return float(ratio.max())

    def finish(self):
        assert self.zmin <= -88.73 and self.zmax >= 88.0, f"{self.family}: z spans only [{self.zmin}, {self.zmax}]"
        far = [(Z_GRID[i], float(d)) for i, d in enumerate(self.near) if not d <= 3.0]
        assert not far, f"{self.family}: no pre-activation within 3 of {far}"
        WORST[self.family] = max(WORST.get(self.family, 0.0), self.worst)
        print(f"activation range, {self.family}: max err / tol {self.worst:.3f}, z in [{self.zmin:.1f}, {self.zmax:.1f}]")
        return self.worst
