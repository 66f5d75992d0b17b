"""host._IndexStream, the index stream MBPSGD.fit and Katyusha.fit consume, against the element-by-element loop of the reference
(minibatch_psgd.nim:98-108, katyusha.nim:108-118): chunk[q] = indices[ii]; ii += 1; if ii >= n: ii = 0; reshuffle.  The
generator is a stand-in with a visible shuffle, so neither the library nor a GPU is needed."""
import numpy as np
import pytest

from nimfm_amd.host import _IndexStream

CHUNKS = 4


class RotatingRng:
    """shuffle rotates the array by one, in place, and counts its calls"""

    def __init__(self):
        self.calls = 0

    def shuffle(self, x):
        x[:] = np.roll(x, -1)
        self.calls += 1


def reference_chunks(n, need, shuffle):
    """-> [(chunk, shuffle calls made by the end of the chunk)]"""
    rng = RotatingRng()
    indices = np.arange(n, dtype=np.int64)
    if shuffle:
        rng.shuffle(indices)
    ii, out = 0, []
    for _ in range(CHUNKS):
        chunk = np.empty(need, dtype=np.int64)
        for q in range(need):
            chunk[q] = indices[ii]
            ii += 1
            if ii >= n:
                ii = 0
                if shuffle:
                    rng.shuffle(indices)
        out.append((chunk, rng.calls))
    return out


# a wrap inside a chunk; the wrap on the last index of a chunk (the reshuffle belongs to that chunk); several wraps in one
# chunk; one pass per chunk
@pytest.mark.parametrize("shuffle", [True, False])
@pytest.mark.parametrize("n,need", [(7, 5), (4, 8), (3, 10), (5, 5)])
def test_walk_matches_the_element_loop(n, need, shuffle):
    rng = RotatingRng()
    stream = _IndexStream(n, need, shuffle, rng)
    assert rng.calls == (1 if shuffle else 0)  # the shuffle at the start, before the first chunk is asked for
    for it, (want, calls) in enumerate(reference_chunks(n, need, shuffle)):
        got = stream.chunk(it)
        assert got.dtype == np.int64 and np.array_equal(got, want), (it, got, want)
        assert rng.calls == calls, (it, rng.calls, calls)


@pytest.mark.parametrize("shuffle", [True, False])
def test_explicit_stream(shuffle):
    n, need = 7, 5
    rng = RotatingRng()
    given = (np.arange(CHUNKS * need) * 3) % n
    stream = _IndexStream(n, need, shuffle, rng, given)
    for it in range(CHUNKS):
        got = stream.chunk(it)
        assert got.dtype == np.int64 and np.array_equal(got, given[it * need:(it + 1) * need])
    assert rng.calls == 0  # the caller's stream replaces the internal shuffle
    short = _IndexStream(n, need, shuffle, rng, given[:-1])
    for it in range(CHUNKS - 1):
        short.chunk(it)
    with pytest.raises(ValueError, match="stream holds fewer than"):
        short.chunk(CHUNKS - 1)
