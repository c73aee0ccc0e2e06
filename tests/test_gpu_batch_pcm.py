"""Spec PK-2 on the GPU: batch_unpack_kernel alone (wsa_debug_batch_unpack) at every format's chunk edges and channel counts, bit for bit
against the host's wsa_pcm_decode; batches fed packed clips against the same batches fed the decoded floats (plain, resampled, mixed-rate,
levels 5 and 13); the device-resident entry inside a captured graph; the refusals."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests.batch_pcm_cases import DTYPE, FORMATS, SAMPLE_BYTES, encode, samples
from webspeechanalyzer_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "g711_expected.json")))
CHUNK = {"f32": 4, "i16": 8, "mulaw": 16, "alaw": 16, "u8": 16, "i24": 16, "i32": 4, "f64": 2}      # samples per 16-byte chunk (i24: per 48-byte group)
SENTINEL = np.float32(-12345.5)


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


def _s(torch):
    return torch.cuda.current_stream().cuda_stream


def unpack(clips, stride, fill):
    """clips: [(format name, channels, frames, channel-0 samples as pcm_decode takes them)] -> one launch of the kernel; the bytes between the
    clips and every other channel hold `fill`.  Returns out [n_clips, stride] (pre-filled with SENTINEL)."""
    L = capi.lib()
    off, blobs = [0], []
    for fmt, ch, n, ch0 in clips:
        sb = SAMPLE_BYTES[fmt]
        raw = np.full((n, ch, sb), fill, np.uint8)
        if n:
            raw[:, 0, :] = np.ascontiguousarray(ch0).view(np.uint8).reshape(n, sb)
        pad = -(n * ch * sb) % 16 + 16                              # up to the next multiple of 16, and one whole chunk of `fill` more
        blobs += [raw.reshape(-1), np.full(pad, fill, np.uint8)]
        off.append(off[-1] + n * ch * sb + pad)
    packed = np.concatenate(blobs)
    off = np.asarray(off, np.uint64)
    fm = np.asarray([capi.pcm_format(c[0]) for c in clips], np.int32)
    chs = np.asarray([c[1] for c in clips], np.uint32)
    nf = np.asarray([c[2] for c in clips], np.uint32)
    out = np.full((len(clips), stride), SENTINEL, np.float32)
    st = L.wsa_debug_batch_unpack(0, packed.ctypes.data, off.ctypes.data, fm.ctypes.data, chs.ctypes.data, nf.ctypes.data, len(clips), out.ctypes.data, stride)
    assert st == 0, st
    return out


@pytest.mark.parametrize("fmt", FORMATS)
def test_kernel_alone_at_the_chunk_edges(torch, fmt):
    c = CHUNK[fmt]
    counts = [0, 1, c - 1, c, c + 1, 2 * c - 1, 2 * c + 1, 256 * c - 1, 256 * c, 256 * c + 1]
    elems = 3 if fmt == "i24" else 1
    clips = []
    for ch in (1, 2, 3, 64):
        for k, n in enumerate(counts):
            ch0 = np.roll(samples(fmt, n + 7, ch), -(k + ch) * elems)[:n * elems]       # the edge values, tiled, every clip starting elsewhere in them
            clips.append((fmt, ch, n, ch0))
    want = [capi.pcm_decode(fmt, ch0) if n else np.zeros(0, np.float32) for _, _, n, ch0 in clips]
    for stride in (256 * c + 4, 256 * c + 5):                       # rows on 16 bytes (float4 stores), and rows that are not (the sample path)
        a = unpack(clips, stride, 0xFF)
        b = unpack(clips, stride, 0x00)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "bytes between the clips or of other channels reached the output"
        for i, (_, ch, n, _) in enumerate(clips):
            assert np.array_equal(a[i, :n].view(np.uint32), want[i].view(np.uint32)), (fmt, ch, n, stride)
            assert np.all(a[i, n:] == SENTINEL), (fmt, ch, n, stride, "floats behind the clip's count were written")


def test_kernel_decodes_every_g711_code_to_the_table_value(torch):
    codes = np.arange(256, dtype=np.uint8)
    out = unpack([("mulaw", 1, 256, codes), ("alaw", 1, 256, codes), ("mulaw", 3, 256, codes), ("alaw", 2, 256, codes)], 256, 0xFF)
    for row, law in enumerate(("mulaw", "alaw", "mulaw", "alaw")):
        assert np.array_equal(out[row].astype(np.float64), np.asarray(GOLD[law], np.float64) / 32768.0), (row, law)


# ---- whole batches

def _tables(b, torch):
    r = b.rows(_s(torch))
    spec, foff = b.spectra(_s(torch))
    r.update(spectra=spec, frame_off=foff)
    return r


def _same_tables(got, want):
    assert set(got) == set(want)
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k], equal_nan=True), k
    assert len(want["meta"]) > 0 and len(want["segments"]) > 0


MIX = [("f32", 2), ("i16", 1), ("mulaw", 1), ("alaw", 1), ("u8", 1), ("i24", 2), ("i32", 1), ("f64", 1)]


@pytest.fixture(scope="module")
def mix_clips(torch):
    """eight clips of 1.2 s at 16 kHz, one per format: (packed arrays, the host's decode of them)"""
    from webspeechanalyzer_amd.synth import synth_clips
    ns = 19200
    x = synth_clips(len(MIX), ns, fs=16000, seed=11, device="cuda").cpu().numpy()
    packed = [encode(x[i], f, ch, 100 + i) for i, (f, ch) in enumerate(MIX)]
    decoded = [capi.pcm_decode(f, p, ch) for p, (f, ch) in zip(packed, MIX)]
    assert all(len(d) == ns for d in decoded)
    return ns, packed, decoded


@pytest.mark.parametrize("level", [5, 13])
def test_packed_batch_equals_the_float_batch(torch, mix_clips, level):
    import webspeechanalyzer_amd as wsa
    ns, packed, decoded = mix_clips
    an = wsa.Analyzer(wsa.Config(output_level=level))
    ref = an.batch([ns] * len(MIX), 16000)
    ref.run_host(decoded, _s(torch))
    want = _tables(ref, torch)
    b = an.batch([ns] * len(MIX), 16000)
    b.run_host_packed(packed, [f for f, _ in MIX], [ch for _, ch in MIX], _s(torch))
    _same_tables(_tables(b, torch), want)
    if level == 13:
        got_cb, want_cb = b.callbacks(_s(torch)), ref.callbacks(_s(torch))
        assert [c["segments_ci"] for c in got_cb] == [c["segments_ci"] for c in want_cb]
    # the same batch object again with the formats in another order: the per-run plan follows the call
    order = list(range(len(MIX)))[::-1]
    ref.run_host([decoded[i] for i in order], _s(torch))
    want = _tables(ref, torch)
    b.run_host_packed([packed[i] for i in order], [MIX[i][0] for i in order], [MIX[i][1] for i in order], _s(torch))
    _same_tables(_tables(b, torch), want)
    b.close(); ref.close(); an.close()


def test_i16_clips_through_the_new_entry_equal_run_host_i16(torch, mix_clips):
    import webspeechanalyzer_amd as wsa
    ns, packed, decoded = mix_clips
    x = [decoded[0], decoded[3], decoded[6][:ns - 3]]
    chans = [1, 2, 3]
    clips = [encode(v, "i16", ch, 7 + ch) for v, ch in zip(x, chans)]
    an = wsa.Analyzer(wsa.Config(output_level=5))
    old = an.batch([len(v) for v in x], 16000)
    old.run_host_i16(clips, chans, _s(torch))
    want = _tables(old, torch)
    new = an.batch([len(v) for v in x], 16000)
    new.run_host_packed(clips, "i16", chans, _s(torch))
    _same_tables(_tables(new, torch), want)
    old.close(); new.close(); an.close()


def test_mixed_rate_and_resampled_batches(torch):
    import webspeechanalyzer_amd as wsa
    from webspeechanalyzer_amd.synth import synth_clips
    an = wsa.Analyzer(wsa.Config(output_level=5))
    rates, kinds = [8000, 44100, 16000], [("mulaw", 1), ("i24", 2), ("f32", 1)]
    ns = [int(1.2 * r) for r in rates]
    packed, decoded = [], []
    for i, (r, n, (f, ch)) in enumerate(zip(rates, ns, kinds)):
        x = synth_clips(1, n, fs=r, seed=40 + i, device="cuda").cpu().numpy()[0]
        packed.append(encode(x, f, ch, 50 + i))
        decoded.append(capi.pcm_decode(f, packed[-1], ch))
    ref = an.batch(ns, rates, resample_to=16000)
    ref.run_host(decoded, _s(torch))
    want, want_pcm = _tables(ref, torch), ref.converted_pcm(_s(torch))
    b = an.batch(ns, rates, resample_to=16000)
    b.run_host_packed(packed, [f for f, _ in kinds], [ch for _, ch in kinds], _s(torch))
    _same_tables(_tables(b, torch), want)
    assert np.array_equal(b.converted_pcm(_s(torch)).view(np.uint32), want_pcm.view(np.uint32))
    b.close(); ref.close()
    # one input rate for all clips (wsa_batch_create_resampled)
    kinds = [("alaw", 2), ("u8", 1)]
    packed, decoded = [], []
    for i, (f, ch) in enumerate(kinds):
        x = synth_clips(1, 9600, fs=8000, seed=60 + i, device="cuda").cpu().numpy()[0]
        packed.append(encode(x, f, ch, 70 + i))
        decoded.append(capi.pcm_decode(f, packed[-1], ch))
    ref = an.batch([9600, 9600], 8000, resample_to=16000)
    ref.run_host(decoded, _s(torch))
    want, want_pcm = _tables(ref, torch), ref.converted_pcm(_s(torch))
    b = an.batch([9600, 9600], 8000, resample_to=16000)
    b.run_host_packed(packed, [f for f, _ in kinds], [ch for _, ch in kinds], _s(torch))
    _same_tables(_tables(b, torch), want)
    assert np.array_equal(b.converted_pcm(_s(torch)).view(np.uint32), want_pcm.view(np.uint32))
    b.close(); ref.close(); an.close()


def test_device_resident_packed_clips_inside_a_captured_graph(torch, mix_clips):
    """wsa_batch_run_packed launches kernels only (the descriptor table and the float staging are made by set_input_format): it is captured like
    wsa_batch_run and replayed on other bytes.  That it allocates nothing is not asserted here: the library's own hipMalloc calls are not seen
    by torch.cuda.memory, and no other test has a way either."""
    import webspeechanalyzer_amd as wsa
    ns, packed, decoded = mix_clips
    pick_a, pick_b = [1, 2, 5, 0], [1, 3, 5, 0]                      # formats i16, G.711, i24 stereo, f32 stereo; run b: other bytes in clip 1 (A-law codes read as mu-law)
    kinds = [MIX[i] for i in pick_a]
    an = wsa.Analyzer(wsa.Config(output_level=5))
    b = an.batch([ns] * len(kinds), 16000)
    b.enable_timing(False)
    with pytest.raises(wsa.WsaError, match="before wsa_batch_set_input_format"):
        b.run_packed(0, _s(torch))
    b.set_input_format([f for f, _ in kinds], [ch for _, ch in kinds])
    off = b.packed_offsets()
    assert off[0] == 0 and np.all(off % 16 == 0) and np.all(np.diff(off.astype(np.int64)) >= [ns * ch * SAMPLE_BYTES[f] for f, ch in kinds])

    def image(pick):
        host = np.full(int(off[-1]), 0xFF, np.uint8)
        for k, i in enumerate(pick):
            raw = packed[i].view(np.uint8)
            host[int(off[k]):int(off[k]) + len(raw)] = raw
        return torch.from_numpy(host)

    def floats(pick):
        return [capi.pcm_decode(kinds[k][0], packed[i].view(DTYPE[kinds[k][0]]), kinds[k][1]) for k, i in enumerate(pick)]

    plain = an.batch([ns] * len(kinds), 16000)
    refs = []
    for pick in (pick_a, pick_b):
        plain.run_host(floats(pick), _s(torch))
        refs.append(_tables(plain, torch))
    assert not np.array_equal(refs[0]["feat"], refs[1]["feat"])
    buf = image(pick_a).cuda()
    assert buf.data_ptr() % 16 == 0
    with pytest.raises(wsa.WsaError, match="not aligned to 16 bytes"):
        b.run_packed(buf.data_ptr() + 4, _s(torch))
    with pytest.raises(wsa.WsaError, match="null packed pointer"):
        b.run_packed(0, _s(torch))
    b.run_packed(buf.data_ptr(), _s(torch))                         # eager first
    _same_tables(_tables(b, torch), refs[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            b.run_packed(buf.data_ptr(), side.cuda_stream)
        for pick, ref in ((pick_b, refs[1]), (pick_a, refs[0])):
            buf.copy_(image(pick))
            g.replay()
            side.synchronize()
            _same_tables(_tables(b, torch), ref)
    plain.close(); b.close(); an.close()


def _workspace_bytes(an, b):
    """the device bytes the batch's arena has handed out so far (wsa_batch_info.workspace_bytes, read again)"""
    info = capi._BatchInfo()
    an._check(an.L.wsa_batch_get_info(b.h, ctypes.byref(info)))
    return info.workspace_bytes


def test_refusals_name_the_clip(torch):
    import webspeechanalyzer_amd as wsa
    an = wsa.Analyzer(wsa.Config(output_level=5))
    b = an.batch([1600, 1600, 1600], 16000)
    clips = [np.zeros(1600 * 65, np.uint8)] * 3
    for bad in (4, 5, 6, 7, 12, -1):
        with pytest.raises(wsa.WsaError, match=r"clip 1: unknown input format %d " % bad):
            b.run_host_packed(clips, [2, bad, 3], None, _s(torch))
        with pytest.raises(wsa.WsaError, match=r"clip 2: unknown input format %d " % bad):
            b.set_input_format([8, 9, bad])
    for bad in (0, 65):
        with pytest.raises(wsa.WsaError, match=r"clip 2: channel count %d outside 1 \.\. 64" % bad):
            b.run_host_packed(clips, "u8", [1, 64, bad], _s(torch))
        with pytest.raises(wsa.WsaError, match=r"clip 0: channel count %d outside 1 \.\. 64" % bad):
            b.set_input_format("mulaw", [bad, 1, 1])
    assert list(b.packed_offsets()) == [0, 0, 0, 0]                 # nothing was planned by a refused call
    assert _workspace_bytes(an, b) == b.info["workspace_bytes"]     # ... and nothing allocated: the plan refuses before the staging buffer and the tables
    with pytest.raises(wsa.WsaError, match="before wsa_batch_set_input_format"):
        b.run_packed(16, _s(torch))
    with pytest.raises(wsa.WsaError, match="takes int32"):
        b.run_host_packed([np.zeros(1600, np.float32)] * 3, "i32", None, _s(torch))
    with pytest.raises(wsa.WsaError, match="clip 1: 100 elements"):
        b.run_host_packed([np.zeros(1600, np.uint8), np.zeros(100, np.uint8), np.zeros(1600, np.uint8)], "u8", None, _s(torch))
    b.set_input_format("u8", None)                                  # an accepted plan allocates the staging buffer and its table
    assert _workspace_bytes(an, b) > b.info["workspace_bytes"] and list(b.packed_offsets()) == [0, 1600, 3200, 4800]
    # streams keep their four formats
    st = an.streams(2, 16000)
    for name in ("u8", "i24", "i32", "f64"):
        with pytest.raises(wsa.WsaError, match=r"unknown input format %d \(WSA_PCM_F32 0, WSA_PCM_I16 1, WSA_PCM_MULAW 2, WSA_PCM_ALAW 3\)" % capi.pcm_format(name)):
            st.set_input_format(name)
    with pytest.raises(wsa.WsaError, match="2 channels with WSA_PCM_F32"):
        st.set_input_format("f32", 2)
    st.close(); b.close(); an.close()
