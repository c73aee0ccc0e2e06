"""Spec PK-3 on the host (no device): wsa_pcm_decode_select against numpy's float32 statement of the rule for every format, channel counts 1, 2,
3, 6 and 64, select 0, channels - 1 and the mix, frame counts 0, 1 and 17; a buffer that ends right behind the selected channel of its last
frame, with an unreadable page behind it; mix inputs that round, overflow and hold NaN in one channel; select 0 against wsa_pcm_decode; the
refusals of the host decode, of the Python entries and of the batch plan, each with its message."""
import ctypes
import mmap
import os

import numpy as np
import pytest

from tests.batch_pcm_cases import FORMATS, f64_values, hashed, i24_bytes, same_bits
from tests.pcm_channel_cases import ELEMS, MIX, SAMPLE_BYTES, frames_matrix, interleaved, pk3, plan
from webspeechanalyzer_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHANNELS = [1, 2, 3, 6, 64]
FRAMES = [0, 1, 17]


@pytest.mark.parametrize("fmt", FORMATS)
def test_decode_select_is_numpys_statement_of_pk3(fmt):
    for ch in CHANNELS:
        for n in FRAMES:
            m = frames_matrix(fmt, n, ch, 5 + ch)
            flat = interleaved(m)
            for sel in sorted({0, ch - 1}) + [MIX]:
                got = capi.pcm_decode(fmt, flat, ch, "mix" if sel == MIX else sel)
                want = pk3(fmt, m, sel)
                assert got.dtype == np.float32 and same_bits(got, want), (fmt, ch, n, sel)
            # select 0 is wsa_pcm_decode, bit for bit (NaN payloads included: both copy or convert the same sample)
            old = np.zeros(n, np.float32)
            assert capi.lib().wsa_pcm_decode(capi.pcm_format(fmt), flat.ctypes.data, n, ch, old.ctypes.data) == 0
            assert np.array_equal(capi.pcm_decode(fmt, flat, ch, 0).view(np.uint32), old.view(np.uint32)), (fmt, ch, n)


@pytest.mark.parametrize("fmt", FORMATS)
def test_nothing_behind_the_selected_channel_of_the_last_frame_is_read(fmt):
    """the buffer ends on the last byte of a readable page; the next page is unreadable"""
    libc = ctypes.CDLL(None, use_errno=True)
    libc.mprotect.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    page = mmap.PAGESIZE
    mem = mmap.mmap(-1, 5 * page)                                    # four readable pages (17 frames of 64 doubles are 8704 bytes), one that is not
    base = ctypes.addressof(ctypes.c_char.from_buffer(mem))
    assert base % page == 0
    assert libc.mprotect(base + 4 * page, page, 0) == 0, ctypes.get_errno()
    try:
        L = capi.lib()
        sb = SAMPLE_BYTES[fmt]
        for ch in (2, 3, 64):
            n = 17
            m = frames_matrix(fmt, n, ch, 9)
            raw = interleaved(m).view(np.uint8)
            for sel in (0, 1, ch - 1, MIX):
                last = ch - 1 if sel == MIX else sel
                size = ((n - 1) * ch + last + 1) * sb                # up to the selected channel of the last frame
                start = base + 4 * page - size
                ctypes.memmove(start, raw.ctypes.data, size)
                out = np.zeros(n, np.float32)
                assert L.wsa_pcm_decode_select(capi.pcm_format(fmt), start, n, ch, sel, out.ctypes.data) == 0
                assert same_bits(out, pk3(fmt, m, sel)), (fmt, ch, sel)
                # the Python entry counts the frames whose selected channel is present
                cut = raw[:size] if fmt == "i24" else interleaved(m)[:size // sb]
                assert len(capi.pcm_decode(fmt, cut, ch, "mix" if sel == MIX else sel)) == n
                if last > 0:
                    shorter = cut[:len(cut) - ELEMS.get(fmt, 1)]
                    assert len(capi.pcm_decode(fmt, shorter, ch, "mix" if sel == MIX else sel)) == n - 1
    finally:
        assert libc.mprotect(base + 4 * page, page, 3) == 0
        del base
        try:
            mem.close()
        except BufferError:
            pass


def _mix(fmt, m):
    return capi.pcm_decode(fmt, interleaved(m), m.shape[1], "mix")


def test_mix_sums_that_round():
    # i24: three and six full-scale-ish samples, sums that need more than 24 bits
    v = (hashed(6 * 512, 91) >> np.uint32(8)).astype(np.int64)
    v[:12] = [0x7FFFFF, 0x7FFFFF, 0x7FFFFF, 0x7FFFFD, 0x7FFFFF, 0x7FFFFB, 0x800000, 0x800000, 0x800001, 0x7FFFFF, 0x000001, 0x7FFFFF]
    for ch in (3, 6):
        m = i24_bytes(v).reshape(-1, ch, 3)
        want = pk3("i24", m, MIX)
        assert same_bits(_mix("i24", m), want)
        x = pk3("i24", m, 0).astype(np.float64) + sum(pk3("i24", m, c).astype(np.float64) for c in range(1, ch))
        assert np.any(x.astype(np.float32).astype(np.float64) != x), "no sum of the case rounds"
    # i32: every term is already rounded, the sums round again
    w = hashed(2 * 1024, 92).view(np.int32)
    w[:4] = [2**31 - 1, 2**31 - 1, -2**31, 2**24 + 1]
    for ch in (2, 64):
        m = w.reshape(-1, ch)
        assert same_bits(_mix("i32", m), pk3("i32", m, MIX))
    # two channels: Web Audio's 0.5 * (L + R)
    m = w.reshape(-1, 2)
    lr = pk3("i32", m, 0) + pk3("i32", m, 1)
    assert same_bits(_mix("i32", m), (np.float32(0.5) * lr).astype(np.float32))


def test_mix_overflow_nan_and_one_channel():
    big = np.array([[3e38, 3e38], [-3e38, -3e38], [3e38, -3e38], [3.5e38, -3.5e38], [1e-40, 1e-40], [-0.0, -0.0]], np.float64)
    got = _mix("f64", big)
    assert same_bits(got, pk3("f64", big, MIX))
    assert got[0] == np.inf and got[1] == -np.inf and got[2] == 0 and np.isnan(got[3]) and np.signbit(got[5])
    # NaN in one channel only: that frame's mix is NaN, the other frames' are not
    m = np.resize(f64_values(with_nan=False), 17 * 3).reshape(17, 3)
    m = m[np.all(np.isfinite(m), axis=1)]
    m[4, 1] = np.nan
    got = _mix("f64", m)
    assert np.isnan(got[4]) and np.isnan(got).sum() == 1 and same_bits(got, pk3("f64", m, MIX))
    f = np.resize(hashed(60, 7).astype(np.float32) / np.float32(2**32), 60).reshape(20, 3)
    f[7, 2] = np.nan
    got = _mix("f32", f)
    assert np.isnan(got[7]) and np.isnan(got).sum() == 1 and same_bits(got, pk3("f32", f, MIX))
    # one channel with the mix is the plain decode, bit for bit — a signalling NaN's payload included
    one = np.array([0x7F800001, 0x7FC00000, 0x80000000, 0x00000001, 0x3F800000], np.uint32).view(np.float32)
    assert np.array_equal(capi.pcm_decode("f32", one, 1, "mix").view(np.uint32), one.view(np.uint32))
    for fmt in FORMATS:
        m = frames_matrix(fmt, 17, 1, 3)
        assert same_bits(capi.pcm_decode(fmt, interleaved(m), 1, "mix"), capi.pcm_decode(fmt, interleaved(m), 1, 0))


def test_the_host_decode_refuses():
    L = capi.lib()
    buf, out = np.zeros(64 * 8 * 2, np.uint8), np.zeros(2, np.float32)
    ok = lambda fmt, ch, sel, n=2, i=buf, o=out: L.wsa_pcm_decode_select(fmt, i.ctypes.data if i is not None else None, n, ch, sel, o.ctypes.data if o is not None else None)
    assert ok(1, 2, 1) == 0 and ok(11, 64, 63) == 0 and ok(1, 2, MIX) == 0 and ok(1, 1, MIX) == 0
    for ch, sel in ((1, 1), (2, 2), (2, 3), (64, 64), (3, 0xFFFFFFFE), (2, 0x80000000)):
        assert ok(1, ch, sel) != 0, (ch, sel)
    for fmt in (4, 5, 6, 7, 12, -1):
        assert ok(fmt, 1, 0) != 0
    assert ok(1, 0, 0) != 0 and ok(1, 65, 0) != 0 and ok(1, 0, MIX) != 0
    assert ok(1, 2, 0, i=None) != 0 and ok(1, 2, 0, o=None) != 0 and ok(1, 2, 0, n=0, i=None, o=None) == 0
    # the Python entry names what it refuses
    a = np.zeros(12, np.int16)
    with pytest.raises(capi.WsaError, match="select 2 is neither a channel below 2 nor 'mix'"):
        capi.pcm_decode("i16", a, 2, 2)
    with pytest.raises(capi.WsaError, match="a channel index or 'mix'"):
        capi.pcm_decode("i16", a, 2, "left")
    with pytest.raises(capi.WsaError, match="a channel index or 'mix'"):
        capi.pcm_decode("i16", a, 2, -1)
    with pytest.raises(capi.WsaError, match=r"channel count 65 outside 1 \.\. 64"):
        capi.pcm_decode("i16", a, 65, 0)
    with pytest.raises(capi.WsaError, match="takes int16"):
        capi.pcm_decode("i16", a.astype(np.float32), 2, 1)


def test_the_batch_plan_lays_sources_out_once_and_refuses_by_clip():
    # stereo i16 source (clip 1) read by clips 0, 1, 3; a mono u8 clip; an empty clip; a 3-channel i24 source behind its consumer
    fm = [0, 1, 8, 0, 2, 0, 9]
    ch = [9, 2, 1, 9, 1, 9, 3]                                      # (a consumer's own format and channel entries are not read)
    sel = [1, 0, 0, MIX, MIX, 2, 0]
    src = [1, 1, 2, 1, 4, 6, 6]
    nf = [100, 101, 33, 7, 0, 50, 50]
    st, off, msg = plan(fm, ch, sel, src, nf)
    assert st == 0 and msg == ""
    assert list(off) == [0, 0, 416, 0, 464, 464, 464, 928], list(off)           # 101 * 4 = 404 -> 416; 33 -> 48; 0; 50 * 9 = 450 -> 464
    st, off, _ = plan(fm, ch, None, None, nf)                       # no select, no source: every clip its own channel 0
    assert st == 0 and np.all(off % 16 == 0) and np.all(np.diff(off.astype(np.int64)) >= 0)
    bad = lambda **k: plan(k.get("fm", fm), k.get("ch", ch), k.get("sel", sel), k.get("src", src), k.get("nf", nf))
    cases = [
        (dict(sel=[2, 0, 0, MIX, MIX, 2, 0]), "clip 0: select 2 is neither a channel below 2 nor WSA_CHANNEL_MIX"),
        (dict(sel=[1, 0, 1, MIX, MIX, 2, 0]), "clip 2: select 1 is neither a channel below 1 nor WSA_CHANNEL_MIX"),
        (dict(sel=[1, 0, 0, MIX, MIX, 3, 0]), "clip 5: select 3 is neither a channel below 3 nor WSA_CHANNEL_MIX"),
        (dict(sel=[1, 0, 0, MIX - 1, MIX, 2, 0]), "clip 3: select 4294967294 is neither a channel below 2 nor WSA_CHANNEL_MIX"),
        (dict(src=[1, 1, 2, 7, 4, 6, 6]), "clip 3: source 7 outside 0 .. 6"),
        (dict(src=[1, 1, 2, 0, 4, 6, 6]), "clip 3: source 0 is not its own source (it reads clip 1)"),
        (dict(src=[1, 1, 2, 1, 4, 6, 5]), "clip 5: source 6 is not its own source (it reads clip 5)"),
        (dict(nf=[102, 101, 33, 7, 0, 50, 50]), "clip 0: 102 frames, its source clip 1 holds 101"),
        (dict(nf=[100, 101, 33, 7, 0, 51, 50]), "clip 5: 51 frames, its source clip 6 holds 50"),
        (dict(fm=[0, 5, 8, 0, 2, 0, 9]), "clip 1: unknown input format 5 (WSA_PCM_F32 0, WSA_PCM_I16 1, WSA_PCM_MULAW 2, WSA_PCM_ALAW 3, WSA_PCM_U8 8, WSA_PCM_I24 9, WSA_PCM_I32 10, WSA_PCM_F64 11)"),
        (dict(ch=[9, 2, 1, 9, 1, 9, 65]), "clip 6: channel count 65 outside 1 .. 64"),
        (dict(ch=[9, 0, 1, 9, 1, 9, 3]), "clip 1: channel count 0 outside 1 .. 64"),
    ]
    for k, want in cases:
        st, _, msg = bad(**k)
        assert st != 0 and msg == want, (k, msg)


def test_the_tile_is_a_multiple_of_16_frames_and_fits_its_budget():
    for fmt in FORMATS:
        for ch in range(1, 65):
            t = capi.pcm_channels_tile_frames(fmt, ch)
            assert t >= 16 and t % 16 == 0 and t <= 2048 and t * ch * SAMPLE_BYTES[fmt] <= 16384, (fmt, ch, t)
    assert capi.pcm_channels_tile_frames("i16", 2) == 2048 and capi.pcm_channels_tile_frames("f64", 64) == 32 and capi.pcm_channels_tile_frames("i24", 3) == 1808
    L = capi.lib()
    assert L.wsa_pcm_channels_tile_frames(5, 2) == 0 and L.wsa_pcm_channels_tile_frames(1, 0) == 0 and L.wsa_pcm_channels_tile_frames(1, 65) == 0


def test_the_new_entries_are_declared_and_the_debug_entry_is_not():
    header = open(os.path.join(ROOT, "include", "wsa.h")).read()
    L = capi.lib()
    for name in ("wsa_pcm_decode_select", "wsa_batch_set_input_channels", "wsa_batch_run_host_channels", "wsa_stream_set_input_channels", "wsa_pcm_channels_tile_frames"):
        assert hasattr(L, name) and name in header and name in capi.ABI_SYMBOLS
    assert "#define WSA_CHANNEL_MIX 0xFFFFFFFFu" in header and capi.CHANNEL_MIX == 0xFFFFFFFF
    assert hasattr(L, "wsa_debug_batch_deinterleave") and "wsa_debug_batch_deinterleave" not in header
