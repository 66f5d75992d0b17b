"""`load` of a model dump whose number blocks are parsed on the device (nimfm_amd/host.py: _DumpText.block -> parseF64 ->
nfm_parse_f64): what comes back is byte-equal to what was dumped and to what the Python lines read,
blocks of host._LOAD_DEVICE_MIN values and more go through parseF64 and smaller ones do not, and a damaged dump behaves as it
does without a device path."""
import io
import contextlib

import numpy as np
import pytest

import nimfm_amd as nf
from nimfm_amd import cli, host

pytestmark = pytest.mark.gpu
T = host._LOAD_DEVICE_MIN


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def wide(rng, shape):
    return rng.standard_normal(shape) * 10.0 ** rng.integers(-9, 9, shape)


def model_of(kind, size, rng):
    """a model whose largest number block has exactly `size` values (size a multiple of 16)"""
    k = 16
    if kind == "fm2":
        fm = nf.newFactorizationMachine("regression", degree=2, nComponents=k, warmStart=True)
        d = size // k
    elif kind == "fm3_explicit":
        fm = nf.newFactorizationMachine("regression", degree=3, nComponents=k, fitLower="explicit", warmStart=True)
        d = size // k
    elif kind == "fm3_augment":
        fm = nf.newFactorizationMachine("classification", degree=3, nComponents=k, fitLower="augment", warmStart=True)
        assert fm.nAugments == 1
        d = size // k - fm.nAugments
    elif kind == "ffm":
        fm = nf.newFieldAwareFactorizationMachine("classification", nComponents=k, warmStart=True)
        d = size // k
        fm.set_params(wide(rng, (3, d, k)), rng.standard_normal(d), -3.5)
        return fm
    else:
        fm = nf.newConvexFactorizationMachine("regression", maxComponents=k + 2)
        d = size // k
        fm.set_params(wide(rng, (k, d)), rng.standard_normal(k), rng.standard_normal(d), 1e-30)
        return fm
    fm.set_params(wide(rng, (fm.nOrders, k, d + fm.nAugments)), rng.standard_normal(d), 0.125)
    fm.lams = rng.standard_normal(k)
    return fm


def same_model(a, b):
    assert type(a) is type(b)
    assert a.P.shape == b.P.shape and np.array_equal(bits(a.P), bits(b.P))
    assert np.array_equal(bits(a.w), bits(b.w))
    assert np.array_equal(bits([a.intercept]), bits([b.intercept]))
    if hasattr(a, "lams"):
        assert np.array_equal(bits(a.lams), bits(b.lams))


def spy(monkeypatch):
    calls, real = [], host.parseF64
    monkeypatch.setattr(host, "parseF64", lambda t, r, c, *a, **kw: (calls.append((r, c)), real(t, r, c, *a, **kw))[1])
    return calls


KINDS = ["fm2", "fm3_explicit", "fm3_augment", "ffm", "cfm"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("size", [T, T - 16], ids=["at_threshold", "below_threshold"])
def test_load_keeps_the_bytes(kind, size, tmp_path, monkeypatch):
    fm = model_of(kind, size, np.random.default_rng(11))
    path = str(tmp_path / "model.txt")
    fm.dump(path)
    calls = spy(monkeypatch)
    back = nf.load(path, False)
    same_model(back, fm)
    blocks = {"fm2": 1, "fm3_explicit": 2, "fm3_augment": 1, "ffm": 3, "cfm": 1}[kind]
    assert calls == ([(fm.P.shape[-2], fm.P.shape[-1])] * blocks if size >= T else []), calls
    n_calls = len(calls)
    monkeypatch.setattr(host, "_LOAD_DEVICE_MIN", 1 << 62)  # the Python lines alone
    same_model(nf.load(path, False), back)
    assert len(calls) == n_calls


def test_small_model_stays_in_python(tmp_path, monkeypatch):
    fm = model_of("fm2", 16 * 7, np.random.default_rng(12))
    path = str(tmp_path / "small.txt")
    fm.dump(path)
    calls = spy(monkeypatch)
    same_model(nf.load(path, False), fm)
    assert calls == []


def test_w_block_on_the_device(tmp_path, monkeypatch):
    """d >= the threshold: the one-line "w:" block goes through parseF64 too"""
    rng = np.random.default_rng(13)
    fm = nf.newFactorizationMachine("regression", degree=2, nComponents=2, warmStart=True)
    fm.set_params(wide(rng, (1, 2, T)), wide(rng, T), 2.5)
    path = str(tmp_path / "w.txt")
    fm.dump(path)
    calls = spy(monkeypatch)
    same_model(nf.load(path, False), fm)
    assert calls == [(2, T), (1, T)]


def outcome(path):
    try:
        m = nf.load(path, False)
    except Exception as e:  # noqa: BLE001 -- the type is what is compared
        return type(e), None
    return None, m


def damaged(text, what, k, d):
    lines = text.split("\n")
    p0 = lines.index("P[0]:") + 1
    if what == "short_row_first":
        lines[p0] = lines[p0].rsplit(" ", 1)[0]
    elif what == "short_row_middle":
        lines[p0 + k // 2] = lines[p0 + k // 2].rsplit(" ", 1)[0]
    elif what == "short_row_last":
        lines[p0 + k - 1] = lines[p0 + k - 1].rsplit(" ", 1)[0]
    elif what == "junk_token":
        toks = lines[p0 + 3].split(" ")
        toks[d // 2] = "1.0x"
        lines[p0 + 3] = " ".join(toks)
    elif what == "underscore_token":  # float() reads "1_0" as 10.0, the device does not decide it
        toks = lines[p0 + 3].split(" ")
        toks[d // 2] = "1_0"
        lines[p0 + 3] = " ".join(toks)
    elif what == "crlf":
        return "\r\n".join(lines)
    elif what == "w_one_short":
        w0 = lines.index("w:") + 1
        lines[w0] = lines[w0].rsplit(" ", 1)[0]
    elif what == "extra_token":
        lines[p0 + 1] += " 77.5"
    elif what == "truncated_file":
        lines = lines[: p0 + k - 2]
    return "\n".join(lines)


@pytest.mark.parametrize("what", ["short_row_first", "short_row_middle", "short_row_last", "junk_token", "underscore_token", "crlf",
                                  "w_one_short", "extra_token", "truncated_file"])
def test_damaged_dump(what, tmp_path, monkeypatch):
    k = 16
    fm = model_of("fm2", T, np.random.default_rng(14))
    path = str(tmp_path / "model.txt")
    fm.dump(path)
    with open(path, newline="") as f:
        text = f.read()
    bad = str(tmp_path / "damaged.txt")
    with open(bad, "w", newline="") as f:
        f.write(damaged(text, what, k, T // k))
    err_dev, m_dev = outcome(bad)
    monkeypatch.setattr(host, "_LOAD_DEVICE_MIN", 1 << 62)
    err_py, m_py = outcome(bad)
    assert err_dev is err_py, (err_dev, err_py)
    if what.startswith("short_row") or what in ("junk_token", "truncated_file"):
        assert err_py is not None
    else:
        assert err_py is None
        same_model(m_dev, m_py)
    if what == "w_one_short":
        assert not m_dev.w.any() and len(m_dev.w) == T // k
    if what in ("crlf", "extra_token"):
        same_model(m_dev, fm)


def test_cli_test_load(tmp_path, monkeypatch):
    rng = np.random.default_rng(15)
    k, d, n = 16, T // 16, 50
    fm = model_of("fm2", T, rng)
    model = str(tmp_path / "model.txt")
    fm.dump(model)
    data = str(tmp_path / "test.svm")
    with open(data, "w") as f:
        for i in range(n):
            cols = np.sort(rng.choice(d, 5, replace=False))
            f.write("%r %s\n" % (float(rng.standard_normal()), " ".join("%d:%r" % (c + 1, float(rng.uniform(-1, 1))) for c in cols)))

    def printed():
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            cli.main(["test", "-t", "r", "--nFeatures", str(d), "--test", data, "--load", model])
        return out.getvalue()

    calls = spy(monkeypatch)
    on_device = printed()
    assert calls == [(k, d)] and "Test RMSE" in on_device
    monkeypatch.setattr(host, "_LOAD_DEVICE_MIN", 1 << 62)
    assert printed() == on_device and len(calls) == 1
