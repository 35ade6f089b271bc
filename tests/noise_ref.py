"""The reg-noise stream of noise_axpy_kernel (csrc/misc_kernels.hip; DESIGN.md "The reg-noise stream") restated in plain
numpy: the reference of tests/test_noise_host.py and tests/test_noise_gpu.py (no test lives here).

Quad q of a call (elements 4q .. 4q+3) is one Philox4x32-10 block:
    counter = {lo32(q + offset), hi32(q + offset), 0, 0}   (q + offset modulo 2^64),   key = {lo32(seed), hi32(seed)}
    u_j = ((w_j >> 8) as float32 + 0.5f) * 2^-24           two IEEE float32 operations; u in (0, 1] (see uniforms)
    element 4q + 2h     = sqrt(-2 ln u_{2h}) * cos(2 pi u_{2h+1})
    element 4q + 2h + 1 = sqrt(-2 ln u_{2h}) * sin(2 pi u_{2h+1})          h = 0, 1
A call of n elements consumes ceil(n / 4) counters."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # Philox4x32 multipliers (words 0 and 2)
W0, W1 = 0x9E3779B9, 0xBB67AE85          # Weyl increments of the key
MASK32 = 0xFFFFFFFF
MASK64 = (1 << 64) - 1


def philox4x32_10(counter_words, key_words, rounds=10):
    """counter_words [..., 4], key_words [..., 2] (broadcast against each other), 32-bit values -> [..., 4] uint32."""
    c = np.asarray(counter_words, dtype=np.uint64) & np.uint64(MASK32)
    k = np.asarray(key_words, dtype=np.uint64) & np.uint64(MASK32)
    lead = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., j], lead).copy() for j in range(4))
    k0, k1 = (np.broadcast_to(k[..., j], lead).copy() for j in range(2))
    m32, s32 = np.uint64(MASK32), np.uint64(32)
    for _ in range(rounds):
        p0 = np.uint64(M0) * c0                       # 32 x 32 -> 64 bits: exact in uint64
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m32, (p0 >> s32) ^ c3 ^ k1, p0 & m32
        k0 = (k0 + np.uint64(W0)) & m32
        k1 = (k1 + np.uint64(W1)) & m32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def uniform(words):
    """32-bit words -> u in float32 by exactly the kernel's two roundings.  (w >> 8) < 2^24 converts exactly; + 0.5f is exact
    below 2^23 and rounds to even from 2^23 up (the grid there is the integers), so the top value 2^24 - 1 becomes 2^24 and
    u == 1.0; the multiplication by 2^-24 is exact.  u lies in [2^-25, 1]."""
    w = np.asarray(words, dtype=np.uint32)
    f = (w >> np.uint32(8)).astype(np.float32)
    return (f + np.float32(0.5)) * np.float32(2.0 ** -24)


def words(n, seed, offset):
    """The [ceil(n / 4), 4] uint32 Philox output words of a call of n elements."""
    seed, offset = int(seed) & MASK64, int(offset) & MASK64
    nq = (int(n) + 3) // 4
    q = np.arange(nq, dtype=np.uint64) + np.uint64(offset)          # wraps modulo 2^64, as the kernel's sum does
    ctr = np.zeros((nq, 4), dtype=np.uint64)
    ctr[:, 0] = q & np.uint64(MASK32)
    ctr[:, 1] = q >> np.uint64(32)
    return philox4x32_10(ctr, np.array([seed & MASK32, seed >> 32], dtype=np.uint64))


def _box_muller(u, dtype):
    u = u.astype(dtype)
    out = np.empty_like(u)
    two_pi = dtype(2.0 * np.pi)
    for h in range(2):
        rad = np.sqrt(dtype(-2.0) * np.log(u[:, 2 * h]))
        ang = two_pi * u[:, 2 * h + 1]
        out[:, 2 * h] = rad * np.cos(ang)
        out[:, 2 * h + 1] = rad * np.sin(ang)
    return out.reshape(-1)


def normals(n, seed, offset):
    """The first n normals of the stream at (seed, offset): float64 evaluation of Box-Muller on the float32 u."""
    return _box_muller(uniform(words(n, seed, offset)), np.float64)[:int(n)]


def normals32(n, seed, offset):
    """The same expression in numpy float32 (np.log / np.sqrt / np.cos / np.sin of float32 arrays): the "precise fp32"
    evaluation whose distance from normals() is the yardstick of the kernel's tolerance."""
    return _box_muller(uniform(words(n, seed, offset)), np.float32)[:int(n)]
