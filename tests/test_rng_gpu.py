"""The Philox mask generator (csrc/rng.hip: sat_rng_fill, sat_rng_fill_segments, sat_counter_add)
against tests/philox_ref.py, bit for bit: element i of stream s under seed k is one fixed word of
Philox-4x32-10, so checkpoint resume and oracle parity rest on more than a keep rate.
tests/test_philox_ref_cpu.py ties the reference to the Random123 known answers."""
import numpy as np
import pytest
import torch

import philox_ref as P

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
HI_SEED = (0x9E3779B9 << 32) | 0x7F4A7C15          # high word set, top bit set
HI_STREAM = (3 << 32) | 11                         # a stream id >= 2^32
GRID = 4 * 256 * 4096                              # elements one pass of sat_rng_fill's grid covers
SEG_GRID = 4 * 256 * 1024                          # ... and of one segment's blocks


def _seed(cuda, seed):
    """The device seed word (int64 storage of the 64-bit pattern)."""
    seed %= 1 << 64
    return torch.tensor([seed - (1 << 64) if seed >= 1 << 63 else seed], dtype=torch.int64,
                        device=cuda)


def _fill(cuda, n, seed, sid, keep, on, pad=8):
    """sat_rng_fill over the first n elements of a NaN buffer with ``pad`` sentinels behind."""
    from sat_amd import kernels as K
    buf = torch.full((n + pad,), float("nan"), device=cuda)
    buf[n:] = SENTINEL
    K.rng_fill(buf[:n], _seed(cuda, seed), sid, keep, on)
    torch.cuda.synchronize()
    assert bool((buf[n:] == SENTINEL).all()), "wrote behind the last element"
    return buf[:n].cpu()


@pytest.mark.parametrize("n,seed,sid,keep", [
    (1, 7, 1, 0.9), (3, HI_SEED, 2, 0.5), (4, 7, HI_STREAM, 0.1), (5, HI_SEED, HI_STREAM, 0.9),
    (1023, 7, 1, 0.5), (1024, HI_SEED, 5, 0.9), (1025, 11, HI_STREAM, 0.1),
    (1025, HI_SEED, HI_STREAM, 0.5), (1025, (1 << 64) - 1, (1 << 64) - 1, 0.9),
    (GRID + 7, HI_SEED, HI_STREAM, 0.9)])           # past the 4096-block grid: the stride loop
def test_rng_fill_is_philox(cuda, n, seed, sid, keep):
    on = 1.0 / keep
    got = _fill(cuda, n, seed, sid, keep, on)
    want = torch.from_numpy(P.mask(n, seed, sid, keep, on))
    assert torch.equal(got, want), int((got != want).sum())


def _segments(cuda, specs, seed, total):
    from sat_amd import kernels as K
    arena = torch.full((total,), SENTINEL, device=cuda)
    K.rng_fill_segments(arena, K.rng_segments(specs), _seed(cuda, seed))
    torch.cuda.synchronize()
    want = np.full(total, SENTINEL, dtype=np.float32)
    for off, n, sid, keep, on in specs:
        want[off:off + n] = P.mask(n, seed, sid, keep, on)
    return arena.cpu(), torch.from_numpy(want)


def test_segments_both_store_paths(cuda):
    """Segments at offsets = 0, 1, 2, 3 mod 4 (the 16-byte store and the scalar one), sizes with
    every n % 4, gaps of sentinel between and behind them left alone."""
    specs, off = [], 0
    for k, n in enumerate((1029, 6, 1027, 1024, 1, 514, 3, 4)):
        off += (k % 4 - off) % 4 + 4                # offset = k mod 4, at least 4 sentinels before
        specs.append((off, n, HI_STREAM + k, (0.9, 0.5, 0.1)[k % 3], 1.0 + k))
        off += n
    assert sorted({s[0] % 4 for s in specs}) == [0, 1, 2, 3]
    got, want = _segments(cuda, specs, HI_SEED, off + 9)
    assert torch.equal(got, want)


def test_segments_stride_loop_and_32(cuda):
    """One segment past the 1024 blocks a segment gets (its stride loop runs) beside small ones,
    32 segments in all -- the most the entry takes."""
    big = SEG_GRID + 4 * 256 + 5
    specs, off = [(1, big, 77, 0.9, 1.0 / 0.9)], 1 + big + 3
    for k in range(31):
        n = 1 + 37 * k
        specs.append((off, n, 100 + k, 0.5, 2.0))
        off += n + (k % 3)
    assert len(specs) == 32
    got, want = _segments(cuda, specs, 12345, off + 4)
    assert torch.equal(got, want)


def test_segments_refusals(cuda):
    from sat_amd import _lib, kernels as K
    arena = torch.full((4096,), SENTINEL, device=cuda)
    seed = _seed(cuda, 1)
    with pytest.raises(_lib.SatLibraryError, match="nseg"):
        K.rng_fill_segments(arena, K.rng_segments([(64 * k, 8, k, 0.5, 1.0) for k in range(33)]),
                            seed)
    with pytest.raises(_lib.SatLibraryError, match="bad segment"):
        K.rng_fill_segments(arena, K.rng_segments([(0, 8, 1, 0.5, 1.0), (-4, 8, 2, 0.5, 1.0)]),
                            seed)
    torch.cuda.synchronize()
    assert bool((arena == SENTINEL).all())


def test_counter_add(cuda):
    """The per-step seed advance: exact 64-bit adds (1, 2^33, a carry out of the low word), and a
    fill after the add draws the reference's mask at seed + 1."""
    from sat_amd import _lib, kernels as K
    c = _seed(cuda, 5)
    _lib.call("sat_counter_add", c.data_ptr(), 1, K._stream())
    _lib.call("sat_counter_add", c.data_ptr(), 1 << 33, K._stream())
    assert int(c.item()) == 5 + 1 + (1 << 33)
    c = _seed(cuda, 0xFFFFFFFF)
    _lib.call("sat_counter_add", c.data_ptr(), 1, K._stream())
    assert int(c.item()) == 1 << 32
    seed = _seed(cuda, HI_SEED)
    _lib.call("sat_counter_add", seed.data_ptr(), 1, K._stream())
    out = torch.full((1027,), float("nan"), device=cuda)
    K.rng_fill(out, seed, 9, 0.5, 2.0)
    torch.cuda.synchronize()
    assert int(seed.item()) % (1 << 64) == HI_SEED + 1
    assert torch.equal(out.cpu(), torch.from_numpy(P.mask(1027, HI_SEED + 1, 9, 0.5, 2.0)))
    assert not np.array_equal(P.mask(1027, HI_SEED + 1, 9, 0.5, 2.0),
                              P.mask(1027, HI_SEED, 9, 0.5, 2.0))


# Found with philox_ref on the CPU (seeds 1.., stream 3, the first 2^20 elements, ~1e8 words
# searched): element 600065 of stream 3 under seed 94 is the word 0xffffff85 >= 2^32 - 128, which
# float32 rounds up to 2^32, so u = 1.0 exactly.
EDGE_SEED, EDGE_STREAM, EDGE_INDEX = 94, 3, 600065


def test_keep_one_keeps_every_element(cuda):
    """A rate-0 mask (keep = 1) is all ones, through both entries, over a range that holds a word
    whose u rounds to 1.0 (u < keep is false there: the generator must not draw for keep >= 1)."""
    from sat_amd import kernels as K
    n = 1 << 20
    w = P.words(n, EDGE_SEED, EDGE_STREAM)
    assert int(w[EDGE_INDEX]) >= 2 ** 32 - 128      # the constant is re-derived, not trusted
    assert not (w.astype(np.float32)[EDGE_INDEX] * np.float32(2.0 ** -32) < np.float32(1.0))
    got = _fill(cuda, n, EDGE_SEED, EDGE_STREAM, 1.0, 1.0)
    assert bool((got == 1.0).all()), torch.nonzero(got != 1.0).flatten().tolist()
    arena = torch.full((n + 16,), SENTINEL, device=cuda)
    K.rng_fill_segments(arena, K.rng_segments([(3, n, EDGE_STREAM, 1.0, 1.0)]),
                        _seed(cuda, EDGE_SEED))
    torch.cuda.synchronize()
    arena = arena.cpu()
    assert bool((arena[3:3 + n] == 1.0).all()), torch.nonzero(arena[3:3 + n] != 1.0).flatten().tolist()
    assert bool((arena[:3] == SENTINEL).all()) and bool((arena[3 + n:] == SENTINEL).all())
    # keep just below 1 still draws: the same element is dropped, as before
    k = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
    got = _fill(cuda, n, EDGE_SEED, EDGE_STREAM, k, 1.0)
    assert torch.equal(got, torch.from_numpy(P.mask(n, EDGE_SEED, EDGE_STREAM, k, 1.0)))
    assert float(got[EDGE_INDEX]) == 0.0
