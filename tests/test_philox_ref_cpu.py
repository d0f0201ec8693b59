"""tests/philox_ref.py (the reference the mask-generator GPU tests compare with bit for bit) is
Philox-4x32-10: it reproduces the Random123 known-answer vectors, and its element mapping and
keep test are what csrc/rng.hip documents."""
import numpy as np

import philox_ref as P

F = 0xFFFFFFFF
# Random123 kat_vectors, philox4x32 10 rounds: counter, key, output
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((F, F, F, F), (F, F), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def _scalar(ctr, key):
    """Python-int restatement of the round function, independent of the vectorised one."""
    c, k = list(ctr), list(key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & F, (p0 >> 32) ^ c[3] ^ k[1], p0 & F]
        k = [(k[0] + 0x9E3779B9) & F, (k[1] + 0xBB67AE85) & F]
    return tuple(c)


def test_known_answers():
    for ctr, key, want in KAT:
        got = tuple(int(x) for x in P.philox4x32_10(*ctr, *key))
        assert got == want, (ctr, key, [hex(x) for x in got])
        assert _scalar(ctr, key) == want


def test_known_answers_vectorised():
    """All three vectors in one call: the array path gives each lane its own answer."""
    cols = [np.array([v[0][j] for v in KAT], dtype=np.uint64) for j in range(4)]
    keys = [np.array([v[1][j] for v in KAT], dtype=np.uint64) for j in range(2)]
    got = np.stack(P.philox4x32_10(*cols, *keys), -1)
    assert got.dtype == np.uint32
    assert [tuple(int(x) for x in row) for row in got] == [v[2] for v in KAT]


def test_words_mapping():
    """Element i is word i % 4 of the block at counter (i // 4, stream id), key = seed; a window
    that starts inside a group equals the same slice of the whole stream."""
    seed, sid = (0x89ABCDEF << 32) | 0x01234567, (5 << 32) | 77
    w = P.words(23, seed, sid)
    for i in (0, 1, 2, 3, 4, 7, 22):
        want = _scalar((i // 4, 0, sid & F, sid >> 32), (seed & F, seed >> 32))[i % 4]
        assert int(w[i]) == want
    assert np.array_equal(P.words(9, seed, sid, start=6), w[6:15])
    # the counter's second word is the group's high half
    big = (1 << 34) + 5
    want = _scalar((big // 4 & F, big // 4 >> 32, sid & F, sid >> 32), (seed & F, seed >> 32))
    assert int(P.words(1, seed, sid, start=big)[0]) == want[big % 4]


def test_mask_draw():
    seed, sid, n = 1234, 7, 4099
    w = P.words(n, seed, sid).astype(np.float64)
    for keep in (0.1, 0.5, 0.9):
        m = P.mask(n, seed, sid, keep, 1.0 / keep)
        assert m.dtype == np.float32 and set(np.unique(m)) <= {np.float32(0), np.float32(1 / keep)}
        # away from the float32 rounding of u the draw is u < keep in exact arithmetic
        u = w / 2.0 ** 32
        clear = np.abs(u - np.float64(np.float32(keep))) > 2.0 ** -23
        assert np.array_equal((m != 0)[clear], (u < keep)[clear])
        assert abs(float((m != 0).mean()) - keep) < 4 * (keep * (1 - keep) / n) ** 0.5


def test_float_edge_of_the_draw():
    """float32(v) rounds the 129 largest words up to 2^32, so u is exactly 1.0 there: the raw
    comparison with keep = 1 would drop them; the mask keeps every element for keep >= 1."""
    inv = np.float32(2.0 ** -32)
    assert not (np.float32(2 ** 32 - 128) * inv < np.float32(1))
    assert np.float32(2 ** 32 - 129) * inv < np.float32(1)
    assert np.all(P.mask(4096, 3, 9, 1.0, 1.0) == 1.0)
