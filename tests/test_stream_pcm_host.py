"""Spec PK-1 on the host (wsa_pcm_decode, no device): every G.711 code against the committed ITU-T tables, every 16-bit value against
x / 32768 in float64, channel 0 out of interleaved frames, and what the Python wrapper refuses."""
import ctypes
import json
import os

import numpy as np
import pytest

from webspeechanalyzer_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "g711_expected.json")))


def test_fixture_is_the_g711_tables():
    assert len(GOLD["mulaw"]) == 256 and len(GOLD["alaw"]) == 256
    assert (max(GOLD["mulaw"]), min(GOLD["mulaw"]), GOLD["mulaw"][0x7F], GOLD["mulaw"][0xFF]) == (32124, -32124, 0, 0)
    assert (max(GOLD["alaw"]), min(GOLD["alaw"]), GOLD["alaw"][0x55], GOLD["alaw"][0xD5]) == (32256, -32256, -8, 8)


@pytest.mark.parametrize("law", ["mulaw", "alaw"])
def test_every_g711_code_decodes_to_the_table_value(law):
    codes = np.arange(256, dtype=np.uint8)
    got = capi.pcm_decode(law, codes)
    want = np.asarray(GOLD[law], np.float64) / 32768.0
    assert got.dtype == np.float32 and got.shape == (256,)
    assert np.array_equal(got.astype(np.float64), want)


def test_every_i16_value_is_x_over_32768_exactly():
    x = np.arange(-32768, 32768, dtype=np.int64).astype(np.int16)
    got = capi.pcm_decode("i16", x)
    assert np.array_equal(got.astype(np.float64), x.astype(np.float64) / 32768.0)


@pytest.mark.parametrize("channels", [1, 2, 3, 64])
@pytest.mark.parametrize("fmt", ["i16", "mulaw", "alaw", "f32"])
def test_channel_zero_is_element_j_times_channels(fmt, channels):
    rng = np.random.default_rng(channels)
    frames = 37
    if fmt == "i16":
        raw = rng.integers(-32768, 32768, frames * channels).astype(np.int16)
    elif fmt == "f32":
        raw = rng.standard_normal(frames * channels).astype(np.float32)
    else:
        raw = rng.integers(0, 256, frames * channels).astype(np.uint8)
    got = capi.pcm_decode(fmt, raw, channels)
    want = capi.pcm_decode(fmt, np.ascontiguousarray(raw[::channels]))
    assert got.shape == (frames,) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # a row that ends right after channel 0 of its last frame still has that frame
    assert np.array_equal(capi.pcm_decode(fmt, raw[:(frames - 1) * channels + 1], channels).view(np.uint32), want.view(np.uint32))


def test_numbers_name_the_same_formats_as_strings():
    codes = np.arange(256, dtype=np.uint8)
    assert (capi.PCM_F32, capi.PCM_I16, capi.PCM_MULAW, capi.PCM_ALAW) == (0, 1, 2, 3)
    assert np.array_equal(capi.pcm_decode(capi.PCM_MULAW, codes), capi.pcm_decode("mulaw", codes))
    assert np.array_equal(capi.pcm_decode(capi.PCM_ALAW, codes), capi.pcm_decode("alaw", codes))
    assert not np.array_equal(capi.pcm_decode("alaw", codes), capi.pcm_decode("mulaw", codes))


@pytest.mark.parametrize("channels", [0, 65])
def test_wrapper_refuses_channel_counts_outside_1_to_64(channels):
    with pytest.raises(capi.WsaError, match="outside 1 .. 64"):
        capi.pcm_decode("i16", np.zeros(130, np.int16), channels)


@pytest.mark.parametrize("fmt", [4, -1, "pcm24", 1.0])
def test_wrapper_refuses_an_unknown_format(fmt):
    with pytest.raises(capi.WsaError, match="unknown input format"):
        capi.pcm_decode(fmt, np.zeros(8, np.int16))


def test_wrapper_refuses_the_wrong_sample_type():
    with pytest.raises(capi.WsaError, match="takes int16"):
        capi.pcm_decode("i16", np.zeros(8, np.uint8))


def test_library_refuses_what_the_wrapper_refuses():
    L = capi.lib()
    x = np.zeros(130, np.int16)
    out = np.zeros(130, np.float32)
    assert L.wsa_pcm_decode(1, x.ctypes.data, 2, 1, out.ctypes.data) == 0
    for fmt, ch in ((4, 1), (-1, 1), (1, 0), (1, 65)):
        assert L.wsa_pcm_decode(fmt, x.ctypes.data, 2, ch, out.ctypes.data) == 1, (fmt, ch)
    assert L.wsa_pcm_decode(1, None, 2, 1, out.ctypes.data) == 1
    assert L.wsa_pcm_decode(1, None, 0, 1, None) == 0
