"""-m gpu: the texts of tests/ingest_edge_cases.py through nf.parseText and the file loaders (ingest.hip) against
oracle/ingest.py, bit for bit: delimiters on every byte of a thread's 64-byte chunk and on both sides of a tile edge, texts
of every length around a tile edge and around one chunk (also straight after a parse that left the recycled block full of
delimiters), rows and runs of empty lines longer than tiles, more lines and entries than one launch has threads, the number
parser's hard tokens as values and as targets with the strtod fix-up list filled from many workgroups, and the refusals with
the byte they name.  What the texts are built to reach is asserted by tests/test_ingest_edge_cases.py (CPU)."""
import functools
import re

import numpy as np
import pytest

import ingest_edge_cases as E
import nimfm_amd as nf
from test_gpu_ingest import same

pytestmark = pytest.mark.gpu
FAMILIES = {"delims_at_every_offset": E.delims_at_every_offset, "long_rows": E.long_rows, "empty_runs": E.empty_runs,
            "hard_numbers": E.hard_numbers}


@functools.lru_cache(maxsize=None)
def expected(text, ffm):
    return E.expect(text, ffm)


def same_nan_by_isnan(ds, y, r, ffm):
    """same() of test_gpu_ingest.py; where the oracle holds a NaN the device must hold one too, whatever its bits"""
    nd, ny = np.isnan(r["data"]), np.isnan(r["y"])
    if nd.any() or ny.any():
        data = ds.to_host()[2]
        assert np.array_equal(np.isnan(data), nd) and np.array_equal(np.isnan(y), ny)
        r = dict(r, data=np.where(nd, data, r["data"]), y=np.where(ny, y, r["y"]))
    same(ds, y, r, ffm)


def parse_and_compare(text, ffm, r, kwargs=None):
    ds, y = nf.parseText(text, withFields=ffm, **(kwargs or {}))
    same_nan_by_isnan(ds, y, r, ffm)


def load_and_compare(path, text, ffm, r):
    path.write_bytes(text if isinstance(text, bytes) else text.encode())
    ds, y = nf.loadFFMFile(str(path)) if ffm else nf.loadSVMLightFile(str(path))
    same_nan_by_isnan(ds, y, r, ffm)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_well_formed_family(family, tmp_path):
    for i, (name, text, ffm, kw) in enumerate(FAMILIES[family]()):
        r = E.expect(text, ffm, **kw)
        try:
            parse_and_compare(text, ffm, r, kw)
            if i == 0 or ffm:  # upload_file and its own len + 64 buffer: one svmlight and the libffm texts of the family
                load_and_compare(tmp_path / (name + ".txt"), text, ffm, r)
        except AssertionError as e:
            raise AssertionError(name) from e


def sweep(ending):
    # longest first: inside one size class of the device-memory cache the block a text is given held the next longer text,
    # whose last bytes lie in this text's padding
    return [c for c in reversed(E.length_sweep()) if c[0] == "length_%d_%s" % (len(c[1]), ending)]


def failures(cases, run):
    """run(text, ffm, r) on every case; -> the names of those that raised, with the first error (so that one run shows
    every length that goes wrong, not the first)"""
    bad = []
    for name, text, ffm, _ in cases:
        try:
            run(text, ffm, expected(text, ffm))
        except (AssertionError, ValueError, nf.NfmError) as e:
            bad.append((name, repr(e)[:120]))
    return bad


@pytest.mark.parametrize("ending", E.ENDINGS)
def test_length_sweep(ending, tmp_path):
    def run(text, ffm, r):
        parse_and_compare(text, ffm, r)
        if len(text) > 80:  # at the tile edge: the file path too
            load_and_compare(tmp_path / "sweep.txt", text, ffm, r)

    cases = sweep(ending)
    assert len(cases) >= len(E.SWEEP_LENGTHS) - 4
    bad = failures(cases, run)
    assert not bad, (len(bad), bad[:5])


@pytest.mark.parametrize("ending", E.ENDINGS)
def test_dirty_padding(ending):
    """every text of the sweep straight after parses of nothing but ':' and '\\n', so that the 64 bytes behind the text --
    load_chunk64 loads up to 15 of them and masks them -- are delimiters.  The issue's 1 MiB of them first; then, since the
    block cache rounds requests up to 256 bytes and hands out the oldest block of the smallest class that fits, as many as
    fill the text's own class, three times over: that reaches up to three cached blocks of the class, and a block keeps
    what was written behind a shorter text's end."""
    big = E.dirt()

    def run(text, ffm, r):
        with pytest.raises(ValueError, match="malformed svmlight text"):
            nf.parseText(big)
        own = E.dirt((len(text) + 64 + 255) // 256 * 256 - 64)
        for _ in range(3):
            with pytest.raises(ValueError, match="malformed svmlight text"):
                nf.parseText(own)
        parse_and_compare(text, ffm, r)

    bad = failures(sweep(ending), run)
    assert not bad, (len(bad), bad[:5])


@pytest.fixture(scope="module")
def big_text():
    return E.beyond_one_pass()


def test_beyond_one_pass_of_every_launch(big_text):
    name, text, ffm, kw, r = big_text
    ds, y = nf.parseText(text, withFields=ffm)
    assert ds.nSamples == E.BEYOND_LINES and ds.nnz == len(r["data"])
    same(ds, y, r, ffm)


def test_beyond_one_pass_from_a_file(big_text, tmp_path):
    """the same text through upload_file: five 32-MiB chunks over its four reader threads"""
    name, text, ffm, kw, r = big_text
    load_and_compare(tmp_path / "big.svm", text, ffm, r)


def test_refusals_name_the_first_bad_line():
    for name, text, ffm, exc, pattern, span in E.refusals():
        with pytest.raises(getattr(nf, exc, None) or ValueError) as info:
            nf.parseText(text, withFields=ffm)
        assert type(info.value).__name__ == exc, (name, info.value)
        m = re.search(pattern, str(info.value))
        assert m, (name, str(info.value))
        if span is not None:
            # both kernels may flag the line, at different bytes: the first byte named lies inside the first malformed line
            assert int(m.group(1)) >= 2 and span[0] <= int(m.group(2)) < span[1], (name, str(info.value), span)


def test_more_flagged_tokens_than_the_fix_list_holds():
    name, text, ffm, exc, pattern, _ = E.too_many_flagged()
    with pytest.raises(nf.NfmError, match=pattern):
        nf.parseText(text, withFields=ffm)
    ds, y = nf.parseText(text[:text.index(b"\n") + 1] * 3)  # the context is usable afterwards
    assert ds.nSamples == 3 and np.array_equal(y, np.full(3, float(E.FLAGGED[0])))
