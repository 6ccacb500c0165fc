"""rt_display_host (include/rt_abi.h; csrc/host/display.cpp over csrc/rt_display.h) against the independent restatement
tests/_display_reference.py: the generated threshold table in exact arithmetic, the bytes around every threshold, the decode
table's round trip, the float64 formula, the special values, both tones, transfers and layout bits, every argument error, and
the stand-alone sanitizer driver (tests/cpp/display_driver.cpp).  No device."""
import ctypes as C
import os
import re
import subprocess
from decimal import Decimal

import numpy as np
import pytest

import _display_reference as R
from conftest import ROOT

F32, U32 = np.float32, np.uint32
INVALID, CAPACITY = -1, -2
CSRC = os.path.join(ROOT, "ray_tracer_2_amd", "csrc")


def _hex_floats(path, macro):
    text = open(path).read()
    body = text[text.index("#define " + macro):]
    body = body[:body.index("\n#", 1)]
    return np.array([float.fromhex(v[:-1]) for v in re.findall(r"0x[0-9a-f.]+p[+-]\d+f", body)], np.float64)


@pytest.fixture(scope="module")
def header_T():
    """T[0 .. 255] of the generated header, as float32."""
    vals = _hex_floats(os.path.join(CSRC, "rt_srgb_encode_lut.h"), "RT_SRGB_ENCODE_T_VALUES")
    assert len(vals) == 256 and vals[0] == 0
    t = vals.astype(F32)
    assert np.array_equal(t.astype(np.float64), vals)   # (every entry is a binary32)
    return t


def _grey(values):
    """An (n, 1, 4) frame with `values` in every colour channel and alpha 1."""
    v = np.asarray(values, F32).reshape(-1, 1, 1)
    return np.concatenate([np.repeat(v, 3, -1), np.ones_like(v)], -1)


def test_header_thresholds_are_exact(header_T):
    """For every k the header's T[k] encodes to >= (k - 1/2) / 255 in 50-digit arithmetic and its predecessor float does not;
    the table is strictly increasing and is the restatement's own (computed from the encoding by bisection)."""
    bits = header_T.view(U32).astype(np.int64)
    assert np.all(np.diff(bits[1:]) > 0)
    for k in range(1, 256):
        want = (Decimal(k) - Decimal("0.5")) / Decimal(255)
        assert R.encode_exact(R.f32_of(bits[k])) >= want, k
        assert R.encode_exact(R.f32_of(bits[k] - 1)) < want, k
    assert np.array_equal(bits.astype(U32), R.thresholds())


def test_generator_writes_the_committed_header():
    r = subprocess.run(["python3", os.path.join(ROOT, "tools", "micro", "gen_srgb_encode_lut.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_bytes_around_every_threshold(rt, header_T):
    bits = header_T.view(U32).astype(np.int64)[1:]
    k = np.arange(1, 256)
    for d, want in ((0, k), (-1, k - 1), (1, k)):
        got = rt.display_host(_grey(R.f32_of((bits + d).astype(U32))))
        assert np.array_equal(got[:, 0, 0], want) and np.array_equal(got[:, 0, 1], want) and np.array_equal(got[:, 0, 2], want), d
        assert np.all(got[:, 0, 3] == 255)


def test_decode_table_returns_to_its_bytes(rt):
    lut = _hex_floats(os.path.join(CSRC, "rt_srgb_lut.h"), "RT_SRGB_LUT_VALUES").astype(F32)
    assert lut.shape == (256,) and lut[0] == 0 and lut[255] == 1
    got = rt.display_host(_grey(lut))
    assert np.array_equal(got[:, 0, :3], np.repeat(np.arange(256)[:, None], 3, 1))
    assert np.array_equal(R.display(_grey(lut)), got)


def test_no_exception_to_the_float64_formula(rt):
    """10^6 seeded floats of [0, 1] and 10^5 of [0, 0.01]: the byte is round(255 srgb(t)) of the float64 formula wherever that
    formula is not within 1e-9 of a half-way point (its own error; no sample is, with these seeds)."""
    rng = np.random.default_rng(2024)
    t = np.concatenate([rng.random(1_000_000, F32), (rng.random(100_000) * 0.01).astype(F32), [F32(0), F32(1)]]).astype(F32)
    want, s255 = R.srgb_byte_f64(t)
    rgb = np.zeros((t.size // 3 + 1) * 3, F32)
    rgb[:t.size] = t
    frame = np.zeros((rgb.size // 3, 1, 4), F32)
    frame[:, 0, :3] = rgb.reshape(-1, 3)
    got = rt.display_host(frame)[:, 0, :3].reshape(-1)[:t.size]
    near_half = np.abs(s255 - np.floor(s255) - 0.5) < 1e-9
    assert not near_half.any()
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]


def test_special_values_in_colour_and_alpha(rt):
    nan, inf = np.nan, np.inf
    sub = 1e-45
    vals = [0.0, -0.0, sub, -sub, 1.1754942e-38, -1.0, -3e38, 1.0, 1.0000001, 2.0, 3e38, inf, -inf, nan, -nan]
    srgb_want = [0, 0, 0, 0, 0, 0, 0, 255, 255, 255, 255, 255, 0, 0, 0]
    f = _grey(vals)
    f[..., 3] = f[..., 0]
    for transfer in ("srgb", "linear"):
        for tone, white in (("clamp", 1.0), ("reinhard", inf)):
            got = rt.display_host(f, transfer=transfer, tone=tone, white=white)
            assert np.array_equal(got[:, 0, 3], srgb_want), (transfer, tone)   # (alpha: LINEAR, no tone)
            if tone == "clamp":
                assert np.array_equal(got[:, 0, 0], srgb_want), (transfer, tone)
            else:   # m / (1 + m): 1 -> 1/2, 2 -> 2/3, 3e38 and +inf (2^64) -> 1
                assert np.array_equal(got[:, 0, 0] == 0, np.array(srgb_want) == 0) and got[10, 0, 0] == 255 and got[11, 0, 0] == 255
            lay = {"srgb": R.SRGB, "linear": R.LINEAR}[transfer]
            assert np.array_equal(got, R.display(f, R.REINHARD if tone == "reinhard" else R.CLAMP, lay, 0, 1.0, white))
    # LINEAR rounds half up at every byte: (k + 0.5) / 255 lands on k or k + 1 by its own rounding, k / 255 on k
    k = np.arange(256)
    got = rt.display_host(_grey((k / 255.0).astype(F32)), transfer="linear")
    assert np.array_equal(got[:, 0, 0], k)
    # a white whose square underflows: +inf for m > 0 (255), NaN at m = 0 (0)
    got = rt.display_host(_grey([0.0, 1e-3, 1.0]), tone="reinhard", white=1e-30)
    assert got[:, 0, 0].tolist() == [0, 255, 255]
    # an exposure scale that is not finite and > 0 counts as 1
    g = _grey([0.25])
    plain = rt.display_host(g, exposure=2.0)
    for s in (nan, inf, -inf, 0.0, -0.0, -2.0):
        assert np.array_equal(rt.display_host(g, exposure=2.0, exposure_scale=s), plain), s
    assert np.array_equal(rt.display_host(g, exposure=2.0, exposure_scale=0.5), rt.display_host(g))
    assert not np.array_equal(rt.display_host(g), plain)


@pytest.mark.parametrize("white", [0.5, 4.0, np.inf])
def test_tones_and_transfers_agree_with_the_restatement(rt, white):
    c = R.hdr_frame()
    assert c.shape == (19, 37, 4)
    scale = np.array([0.37], F32)
    for tone, tname in ((R.CLAMP, "clamp"), (R.REINHARD, "reinhard")):
        for transfer, xname in ((R.SRGB, "srgb"), (R.LINEAR, "linear")):
            for exposure in (1.0, 2.0 ** -12, 2.0 ** 9, 0.7):
                for s in (None, scale):
                    got = rt.display_host(c, tone=tname, transfer=xname, exposure=exposure, white=white, exposure_scale=s)
                    want = R.display(c, tone, transfer, 0, exposure, white, s)
                    assert got.dtype == np.uint8 and got.shape == (19, 37, 4)
                    assert np.array_equal(got, want), (tname, xname, exposure, np.argwhere(got != want)[:4].tolist())
    # the curve does something: Reinhard differs from the clamp, and between whites
    assert not np.array_equal(rt.display_host(c, tone="reinhard", white=white), rt.display_host(c))


def test_layout_bits_are_the_two_permutations(rt):
    c = R.hdr_frame()
    base = rt.display_host(c, tone="reinhard", white=4.0)
    assert len(np.unique(base[..., 0].astype(int) - base[..., 2])) > 1
    assert np.array_equal(rt.display_host(c, tone="reinhard", white=4.0, bgra=True), base[..., [2, 1, 0, 3]])
    assert np.array_equal(rt.display_host(c, tone="reinhard", white=4.0, top_first=True), base[::-1])
    assert np.array_equal(rt.display_host(c, tone="reinhard", white=4.0, bgra=True, top_first=True), base[::-1][..., [2, 1, 0, 3]])
    for lay in range(4):
        assert np.array_equal(rt.display_host(c, bgra=bool(lay & 1), top_first=bool(lay & 2)), R.display(c, layout=lay)), lay
    # the window: CLAMP, SRGB, B G R A, exposure 1 -- clamp, encode, round, swap
    w = rt.display_host(R.threshold_frame(7, 3), bgra=True)
    assert np.array_equal(w, R.display(R.threshold_frame(7, 3), R.CLAMP, R.SRGB, R.BGRA))


MARK = 0xA5
W, H = 5, 3


def _desc(A, color_plane, out_plane, **over):
    d = A.DisplayDesc(struct_bytes=C.sizeof(A.DisplayDesc), width=W, height=H, exposure=1.0, white=1.0)
    for k, v in dict(dict(color=color_plane.ctypes.data, out=out_plane.ctypes.data), **over).items():
        setattr(d, k, v)
    return d


nan, inf = float("nan"), float("inf")
CASES = [
    ("struct_bytes too small", dict(struct_bytes=56), INVALID, "struct_bytes"),
    ("struct_bytes zero", dict(struct_bytes=0), INVALID, "struct_bytes"),
    ("struct_bytes too large", dict(struct_bytes=72), INVALID, "struct_bytes"),
    ("_p0", dict(_p0=1), INVALID, "_p0"),
    ("_p1", dict(_p1=1), INVALID, "_p1"),
    ("zero width", dict(width=0), INVALID, "zero"),
    ("zero height", dict(height=0), INVALID, "zero"),
    ("unknown tone", dict(tone=2), INVALID, "tone"),
    ("unknown transfer", dict(transfer=2), INVALID, "transfer"),
    ("unknown layout bit", dict(layout=4), INVALID, "layout"),
    ("high layout bit", dict(layout=0x80000001), INVALID, "layout"),
    ("exposure zero", dict(exposure=0.0), INVALID, "exposure"),
    ("exposure negative", dict(exposure=-1.0), INVALID, "exposure"),
    ("exposure NaN", dict(exposure=nan), INVALID, "exposure"),
    ("exposure infinite", dict(exposure=inf), INVALID, "exposure"),
    ("white zero", dict(tone=1, white=0.0), INVALID, "white"),
    ("white negative", dict(tone=1, white=-1.0), INVALID, "white"),
    ("white NaN", dict(tone=1, white=nan), INVALID, "white"),
    ("null color", dict(color=None), INVALID, "color"),
    ("null out", dict(out=None), INVALID, "out"),
    ("2^31 texels", dict(width=1 << 16, height=1 << 15), CAPACITY, "2^31"),
    ("more than 2^31 texels", dict(width=0x7fffffff, height=2), CAPACITY, "2^31"),
]


@pytest.mark.parametrize("what,over,code,text", CASES, ids=[c[0] for c in CASES])
def test_errors_leave_out_untouched(rt, what, over, code, text):
    from ray_tracer_2_amd import _abi as A
    L = rt.load()
    color, out = np.ones((H, W, 4), F32), np.full((H, W, 4), MARK, np.uint8)
    assert L.rt_display_host(C.byref(_desc(A, color, out, **over))) == code, what
    assert text in L.rt_last_error(None).decode(), (what, L.rt_last_error(None))
    assert np.all(out == MARK), what


def test_null_desc_the_call_that_is_right_and_the_wrapper(rt):
    from ray_tracer_2_amd import _abi as A
    L = rt.load()
    assert L.rt_display_host(None) == INVALID and "null" in L.rt_last_error(None).decode()
    color, out = np.ones((H, W, 4), F32), np.full((H, W, 4), MARK, np.uint8)
    # white is ignored by CLAMP, +inf is allowed by REINHARD
    for over in (dict(), dict(white=nan), dict(white=-1.0), dict(tone=1, white=inf), dict(layout=3), dict(transfer=1)):
        out[:] = MARK
        assert L.rt_display_host(C.byref(_desc(A, color, out, **over))) == 0, over
        assert np.all(out == (188 if over.get("tone") else 255) * np.array([1, 1, 1, 0]) + np.array([0, 0, 0, 255])), over   # (1 / (1 + 1) encodes to 188)
    mine = np.zeros((H, W, 4), np.uint8)
    assert rt.display_host(color, out=mine) is mine and np.all(mine == 255)
    for bad in (dict(out=np.zeros((H, W, 4), F32)), dict(out=np.zeros((H, W + 1, 4), np.uint8)), dict(tone="filmic"), dict(transfer="pq"),
                dict(exposure_scale=[1.0, 2.0])):
        with pytest.raises(ValueError):
            rt.display_host(color, **bad)
    with pytest.raises(ValueError):
        rt.display_host(None)
    with pytest.raises(rt.RtError) as e:
        rt.display_host(color, exposure=0.0)
    assert e.value.code == INVALID


def test_sanitizer_driver(rt, tmp_path):
    """tests/cpp/display_driver.cpp with host/display.cpp under AddressSanitizer and UndefinedBehaviorSanitizer, a program of
    its own: both host functions at 1x1, 7x3 and 257x5 on exactly sized heap buffers with every optional pointer on and off,
    and display_host's byte over every float of [0, 1] (on up to eight threads) -- monotone, 255 steps, each at the table's value.  The 7x3 outputs it
    prints are the wrapper's."""
    exe = tmp_path / "display_driver"
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "display_driver.cpp"),
                    os.path.join(CSRC, "host", "display.cpp"), "-o", str(exe)], check=True)
    res = tmp_path / "out.bin"
    run = subprocess.run([str(exe), str(res)], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout, run.stderr)
    for size in ("1x1", "7x3", "257x5"):
        assert f"{size} ok" in run.stdout, run.stdout
    assert "sweep ok: 255 steps" in run.stdout, run.stdout
    # the driver's 7x3 frame is ramp(i) = 2^(i % 40 - 20) * (1 + (i % 7) / 8) over the 84 floats, alpha included
    i = np.arange(7 * 3 * 4)
    frame = (np.exp2((i % 40) - 20.0) * (1 + (i % 7) / 8.0)).astype(F32).reshape(3, 7, 4)
    raw = np.fromfile(res, np.uint8)
    assert raw.size == 7 * 3 * 4 + 4 + 1024
    got_bytes, got_scale, got_hist = raw[:84].reshape(3, 7, 4), raw[84:88].view(F32), raw[88:].view(U32)
    scale, hist = rt.auto_exposure_host(frame, low_permille=100, high_permille=900, key=0.18, min_scale=2.0 ** -8, max_scale=2.0 ** 8, histogram=True)
    assert np.array_equal(got_hist, hist) and got_scale.view(U32)[0] == scale.view(U32)[0]
    want = rt.display_host(frame, tone="reinhard", white=4.0, bgra=True, top_first=True, exposure=1.5, exposure_scale=scale)
    assert np.array_equal(got_bytes, want)
