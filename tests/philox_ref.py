"""Plain numpy Philox-4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3",
SC'11; the Random123 constants) and the mask generator's mapping from (seed, stream id, element
index) to a mask value, restated independently of csrc/rng.hip:

    group g = i // 4, counter = (g lo, g hi, stream lo, stream hi), key = (seed lo, seed hi),
    element i takes word j = i % 4 of the block, and is on iff
    float32(word) * float32(2^-32) < float32(keep); keep >= 1 keeps every element.

All arithmetic is uint64 products split into 32-bit halves, vectorised over any leading shape.
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)      # Weyl key schedule
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """10 rounds over broadcastable uint32-valued arrays; returns four uint32 arrays."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(x).astype(np.uint64) & _LO
                              for x in (c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                           # < 2^64: exact in uint64
        c0, c1, c2, c3 = ((p1 >> _S32) ^ c1 ^ k0, p1 & _LO, (p0 >> _S32) ^ c3 ^ k1, p0 & _LO)
        k0, k1 = (k0 + W0) & _LO, (k1 + W1) & _LO
    return tuple(x.astype(np.uint32) for x in (c0, c1, c2, c3))


def words(n, seed, stream_id, start=0):
    """The uint32 word of elements start .. start + n - 1 of stream ``stream_id`` under ``seed``
    (both taken modulo 2^64)."""
    seed, stream_id = int(seed) % (1 << 64), int(stream_id) % (1 << 64)
    g0, g1 = start // 4, (start + n + 3) // 4
    g = np.arange(g0, g1, dtype=np.uint64)
    r = philox4x32_10(g & _LO, g >> _S32, stream_id & 0xFFFFFFFF, stream_id >> 32,
                      seed & 0xFFFFFFFF, seed >> 32)
    flat = np.stack(np.broadcast_arrays(*r), -1).reshape(-1)
    return flat[start - 4 * g0:start - 4 * g0 + n]


def mask(n, seed, stream_id, keep, on):
    """float32 [n]: the mask sat_rng_fill(out, n, seed, stream_id, keep, on) is to draw."""
    w = words(n, seed, stream_id)
    keep32 = np.float32(keep)
    if keep32 >= np.float32(1.0):
        kept = np.ones(n, dtype=bool)
    else:
        kept = w.astype(np.float32) * np.float32(2.0 ** -32) < keep32
    return np.where(kept, np.float32(on), np.float32(0.0)).astype(np.float32)
