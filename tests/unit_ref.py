"""Float64 reference of the layer's front-end STAGE alone (features.hip: unit_rows_kernel,
unit_grad_kernel), with derived elementwise error bounds -- a test helper, not a test (numpy only;
never imported by the product).

The yardstick of tests/test_gpu_unit_features.py (pinned on the CPU, against torch and against an
fp32 emulation, by tests/test_unit_ref_cpu.py).  For a row z of d elements, widened exactly to
float64:

    forward_ref(z):         r = 1 / max(|z|, 1e-12),   x = z r          (F.normalize's clamp)
    backward_ref(g, x, r):  out = r (g - x (x . g)),  or  out = r g  on a clamped row (r >= 1e12)

backward_ref takes the KERNEL'S OWN fp32 X and rnorm, widened to float64: the backward stage is
judged on what it read, not on the forward's error.

Bounds (u = 2^-24, the unit roundoff of fp32; first order in u, any summation order):

  forward    |X - x| <= (d + 8) u |x|  per element, and |rnorm - r| <= (d + 8) u r.
             s = sum a_k^2 carries one rounding per product and at most d - 1 per path through the
             sum: relative error <= d u, halved by the square root: d u / 2.  Then one rounding each
             for sqrtf, the division and the scale a_k r: <= (d / 2 + 3) u.  The bound leaves the
             other d / 2 + 5 for the second-order terms.  Inputs must be free of underflow (a
             product a_k^2 below 2^-126 loses relative accuracy); the clamped rows are exempt from
             that: their r is 1e12 whatever s was rounded to.
  backward   |out_k - ref_k| <= r (d + 8) u (|g_k| + |x_k| sum_j |x_j g_j|), before the rounding to
             Z's type.  t = sum x_j g_j: <= d u sum |x_j g_j|; x_k t, the subtraction and the scale
             by r add three roundings on |g_k| + |x_k| sum |x_j g_j| at most: (d + 3) u, with 5 u
             left for second order.  A clamped row is one multiplication: fl(r g_k) exactly.
  rounding   to Z's type adds 2^-8 |ref_k| (bf16) or 2^-11 |ref_k| (fp16), nothing for fp32.  Below
             the type's smallest normal number the spacing no longer shrinks with the value, so the
             term is never less than half the subnormal spacing: 2^-25 for fp16 (its subnormals
             are multiples of 2^-24; a row of 65504s has r < 2^-16 and a gradient down there),
             2^-134 for bf16.  An fp16 result past 65504 is inf, as torch's cast gives.

Both bounds are derived, not measured; tests/test_unit_ref_cpu.py evaluates the same formulas in
numpy float32 with plain sequential summation (the worst order) and pins how much of each bound
that uses.
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24          # unit roundoff of fp32
CLAMP = 1e-12           # F.normalize's eps
# (relative rounding, half the subnormal spacing) of the output type
ROUNDING = {"float32": (0.0, 0.0), "bfloat16": (2.0 ** -8, 2.0 ** -134),
            "float16": (2.0 ** -11, 2.0 ** -25)}

# (rows, d) of the GPU stage tests: d = 1, below / at / past a 16-B vector of either width, odd d
# (misaligned half rows), d % 4 != 0 (misaligned fp32 rows), more rows than a workgroup holds
# (257 = 64 workgroups + 1 row), every STEPS instantiation (d <= 256, 512, 1024, 2048, 4096 for
# fp32; <= 512 ... 4096 for the half types; d = 1000 is there for fp32's 513 .. 1024 and the half
# types' 513 .. 1024, which no other shape reaches) and the ABI's limit.
SHAPES = [(1, 1), (3, 2), (5, 3), (4, 7), (257, 8), (5, 64), (3, 100), (5, 129), (2, 512),
          (2, 1000), (3, 1028), (2, 4096)]


def forward_ref(z):
    """x, r of rows z (rows x d, any float dtype, widened to float64)."""
    z = np.asarray(z, dtype=np.float64)
    nrm = np.sqrt(np.sum(z * z, axis=-1))
    r = 1.0 / np.maximum(nrm, CLAMP)
    return z * r[..., None], r


def clamped(r):
    """Rows the backward treats as clamped (the kernel's test on its own fp32 rnorm)."""
    return np.asarray(r, dtype=np.float32) >= np.float32(1e12)


def backward_ref(g, x, r):
    """dloss/dz from g = dloss/dx, with x and r as the forward left them (float64)."""
    g = np.asarray(g, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    r64 = np.asarray(r, dtype=np.float64)
    t = np.sum(x * g, axis=-1, keepdims=True)
    t = np.where(clamped(r)[..., None], 0.0, t)
    return r64[..., None] * (g - x * t)


def forward_bound(x_ref, d):
    return (d + 8) * U * np.abs(x_ref)


def backward_bound(g, x, r, dtype="float32"):
    """Elementwise bound on |gZ - backward_ref|: the fp32 evaluation plus the rounding to dtype."""
    g = np.asarray(g, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    r64 = np.asarray(r, dtype=np.float64)[..., None]
    d = g.shape[-1]
    sabs = np.sum(np.abs(x * g), axis=-1, keepdims=True)
    b = r64 * (d + 8) * U * (np.abs(g) + np.abs(x) * sabs)
    rel, floor = ROUNDING[dtype]
    if rel:
        b = b + np.maximum(rel * np.abs(backward_ref(g, x, r)), floor)
    return b


def rows_input(rows, d, seed, dtype="float32"):
    """Feature rows of the stage tests (float32 values; the caller casts to `dtype`): standard
    normals scaled per row over four decades, then the special rows where they fit:
      row 0     zero                     -> X = 0, rnorm = 1e12 (clamped)
      row 1     one-hot at d // 2        -> X exact, rnorm = 1
      row 2     1e-20 at 0 (fp32 only)   -> clamped: X = 1e-8
      row 3     65504s (fp16 only)       -> the largest fp16 norm"""
    rng = np.random.Generator(np.random.PCG64(seed))
    z = rng.standard_normal((rows, d)) * 10.0 ** rng.uniform(-2, 2, size=(rows, 1))
    z = z.astype(np.float32)
    if rows > 1:
        z[0] = 0.0
    if rows > 2:
        z[1] = 0.0
        z[1, d // 2] = 1.0
    if rows > 3 and dtype == "float32":
        z[2] = 0.0
        z[2, 0] = 1e-20
    if rows > 4 and dtype == "float16":
        z[3] = 65504.0
    return z


def emulate_forward_f32(z):
    """The forward in numpy float32, one rounding per operation, plain sequential sum."""
    z = np.asarray(z, dtype=np.float32)
    s = np.zeros(z.shape[0], dtype=np.float32)
    for k in range(z.shape[1]):
        s = (s + z[:, k] * z[:, k]).astype(np.float32)
    nrm = np.sqrt(s).astype(np.float32)
    r = (np.float32(1.0) / np.maximum(nrm, np.float32(1e-12))).astype(np.float32)
    return (z * r[:, None]).astype(np.float32), r


def emulate_backward_f32(g, x, r):
    """The backward in numpy float32 (before the output rounding), sequential sum."""
    g = np.asarray(g, dtype=np.float32)
    x = np.asarray(x, dtype=np.float32)
    r = np.asarray(r, dtype=np.float32)
    t = np.zeros(g.shape[0], dtype=np.float32)
    for k in range(g.shape[1]):
        t = (t + x[:, k] * g[:, k]).astype(np.float32)
    t = np.where(clamped(r), np.float32(0.0), t)
    xt = (x * t[:, None]).astype(np.float32)
    return (r[:, None] * (g - xt).astype(np.float32)).astype(np.float32)
