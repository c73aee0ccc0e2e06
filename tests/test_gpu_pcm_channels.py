"""Spec PK-3 on the GPU: batch_deinterleave_kernel alone (wsa_debug_batch_deinterleave) at the tile's edges for every format and channel
counts 2, 3, 6 and 64, rows that do not start on 16 bytes, poisoned bytes behind every source; whole batches whose clips take a channel or
the mix of shared sources against the same Analyzer fed the host-decoded mono floats through run_host (spectra and rows, bit for bit: plain,
resampled, mixed-rate at level 13, run_packed inside a captured graph); stream sets whose streams share packed rows against the float set."""
import ctypes

import numpy as np
import pytest

from tests.batch_pcm_cases import FORMATS, encode, same_bits
from tests.pcm_channel_cases import DTYPE, ELEMS, MIX, SAMPLE_BYTES, frames_matrix, interleaved, pk3, plan
from webspeechanalyzer_amd import capi

pytestmark = pytest.mark.gpu
SENTINEL = np.float32(-12345.5)


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


def _s(torch):
    return torch.cuda.current_stream().cuda_stream


def _name(sel):
    return "mix" if sel == MIX else sel


# ---- the kernel alone

def deinterleave(clips, stride, fill):
    """clips: [(format name, channels, select, source, frames, the source's bytes or None)] -> one launch of the kernel.  The packed buffer is
    exactly as long as the plan says; every byte of it that belongs to no source's frames holds `fill`.  -> out [n_clips, stride]"""
    L = capi.lib()
    fm = np.asarray([capi.pcm_format(c[0]) for c in clips], np.int32)
    ch, sel, src, nf = (np.asarray([c[k] for c in clips], np.uint32) for k in (1, 2, 3, 4))
    st, off, msg = plan(fm, ch, sel, src, nf)
    assert st == 0, msg
    packed = np.full(int(off[-1]), fill, np.uint8)
    for i, c in enumerate(clips):
        if c[3] == i and c[4]:
            raw = np.ascontiguousarray(c[5]).view(np.uint8).reshape(-1)
            assert len(raw) == c[4] * c[1] * SAMPLE_BYTES[c[0]]
            packed[int(off[i]):int(off[i]) + len(raw)] = raw
    out = np.full((len(clips), stride), SENTINEL, np.float32)
    off2 = np.zeros(len(clips) + 1, np.uint64)
    st = L.wsa_debug_batch_deinterleave(0, packed.ctypes.data, len(packed), fm.ctypes.data, ch.ctypes.data, sel.ctypes.data, src.ctypes.data, nf.ctypes.data,
                                        len(clips), off2.ctypes.data, out.ctypes.data, stride, None, 0)
    assert st == 0, st
    assert np.array_equal(off, off2)
    return out


@pytest.mark.parametrize("fmt", FORMATS)
def test_kernel_alone_at_the_tile_edges(torch, fmt):
    """per (channels, frames): the source takes its last channel, a consumer the mix of all frames, a consumer channel 0 of the first half"""
    clips, want = [], []
    longest = 0
    for ch in (2, 3, 6, 64):
        T = capi.pcm_channels_tile_frames(fmt, ch)
        assert T % 16 == 0 and T >= 16
        for n in (0, 1, 15, 16, 17, T - 1, T, T + 1, 2 * T + 3):
            m = frames_matrix(fmt, n, ch, ch + n % 7)
            s = len(clips)
            clips += [(fmt, 1, MIX, s + 1, n, None), (fmt, ch, ch - 1, s + 1, n, interleaved(m)), (fmt, 1, 0, s + 1, n // 2, None)]    # (consumers' own channel entries are not read)
            want += [pk3(fmt, m, MIX), pk3(fmt, m, ch - 1), pk3(fmt, m[:n // 2], 0)]
            # the host's own decode says the same (the CPU tests hold it against numpy on small cases; here at the tile's sizes)
            assert same_bits(capi.pcm_decode(fmt, interleaved(m), ch, "mix"), want[-3]) and same_bits(capi.pcm_decode(fmt, interleaved(m), ch, ch - 1), want[-2])
            longest = max(longest, n)
    for stride in (longest + 1 + (-(longest + 1) % 4), longest + 2 + (-(longest + 1) % 4)):           # rows on 16 bytes, and rows that are not
        a = deinterleave(clips, stride, 0xFF)                       # 0xFF..: NaN as f32 / f64, -1 as the integers;  0x7F..: near full scale, NaN as f32 0x7F7F7F7F is 3.4e38
        b = deinterleave(clips, stride, 0x7F)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "bytes behind a source's last frame reached the output"
        for i, c in enumerate(clips):
            n = c[4]
            if c[2] == MIX:                                         # (a NaN's payload out of an addition is not specified)
                assert same_bits(a[i, :n], want[i]), (fmt, c[1], n, stride, "mix")
            else:
                assert np.array_equal(a[i, :n].view(np.uint32), want[i].view(np.uint32)), (fmt, clips[c[3]][1], c[2], n, stride)
            assert np.all(a[i, n:] == SENTINEL), (fmt, i, n, stride, "floats behind the clip's count were written")


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


def _speech(torch, n, ns, fs, seed):
    from webspeechanalyzer_amd.synth import synth_clips
    return synth_clips(n, ns, fs=fs, seed=seed, device="cuda").cpu().numpy()


def _file(x_by_channel, fmt, seed):
    """float signals, one per channel -> the interleaved samples of a file in that encoding (as pcm_decode takes them)"""
    cols = [encode(x, fmt, 1, seed + c) for c, x in enumerate(x_by_channel)]
    e = ELEMS.get(fmt, 1)
    return np.stack([c.reshape(len(x_by_channel[0]), e) for c in cols], axis=1).reshape(-1)


def _decoded(spec, files):
    """what each clip of `spec` = [(format, channels, select, source, frames)] analyses: the host's decode of its source's file"""
    return [capi.pcm_decode(spec[s][0], files[s], spec[s][1], _name(sel))[:n] for (_, _, sel, s, n) in spec]


def _args(spec):
    return [c[0] for c in spec], [c[1] for c in spec], [_name(c[2]) for c in spec], [c[3] for c in spec]


@pytest.mark.parametrize("fmt", FORMATS)
def test_spectra_at_the_tile_edges_equal_the_float_batch(torch, fmt):
    """the kernel test's shapes through a whole batch: per (channels, frames) the source takes its last channel and a consumer the mix; spectra, frame
    offsets and every row table against the same Analyzer fed the host-decoded floats.  (Clips shorter than one analysis window have no frame on
    either side; their floats are held bit for bit by the kernel test above.)"""
    import webspeechanalyzer_amd as wsa
    rng = np.random.default_rng(capi.pcm_format(fmt))
    spec, files = [], {}
    for ch in (2, 3, 6, 64):
        T = capi.pcm_channels_tile_frames(fmt, ch)
        for n in (0, 1, 15, 16, 17, T - 1, T, T + 1, 2 * T + 3):
            s = len(spec)
            spec += [(fmt, ch, ch - 1, s, n), (fmt, ch, MIX, s, n)]
            files[s] = _file([rng.uniform(-0.9, 0.9, n) for _ in range(ch)], fmt, s) if n else np.zeros(0, DTYPE[fmt])
    decoded = _decoded(spec, files)
    fm, ch, sel, src = _args(spec)
    ns = [c[4] for c in spec]
    an = wsa.Analyzer(wsa.Config(output_level=5))
    ref = an.batch(ns, 16000)
    ref.run_host(decoded, _s(torch))
    want = _tables(ref, torch)
    b = an.batch(ns, 16000)
    b.run_host_channels([files.get(i) for i in range(len(spec))], fm, ch, sel, src, _s(torch))
    got = _tables(b, torch)
    assert set(got) == set(want) and len(want["spectra"]) > 0
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k], equal_nan=True), (fmt, k)
    b.close(); ref.close(); an.close()


@pytest.fixture(scope="module")
def fan_out(torch):
    """a stereo i16 call (two speakers) read by four clips — channel 0, channel 1, the mix and a shorter look at channel 1 —, a 3-channel i24 file
    read by its mix alone, a mono mu-law clip, an empty clip: (spec, files by clip index, decoded floats)"""
    ns = 19200
    x = _speech(torch, 6, ns, 16000, 21)
    spec = [("i16", 2, MIX, 2, ns), ("i16", 2, 0, 2, ns), ("i16", 2, 1, 2, ns), ("mulaw", 1, 0, 3, ns), ("i16", 2, 1, 2, ns - 4001),
            ("i24", 3, MIX, 5, ns), ("u8", 1, MIX, 6, 0)]
    files = {2: _file([x[0], x[1]], "i16", 1), 3: _file([x[2]], "mulaw", 2), 5: _file([x[3], x[4], x[5]], "i24", 3), 6: np.zeros(0, np.uint8)}
    return spec, files, _decoded(spec, files)


def _shuffled(spec, files, decoded, order):
    """the same clips in another order (sources renumbered)"""
    pos = {old: new for new, old in enumerate(order)}
    sp = [(spec[o][0], spec[o][1], spec[o][2], pos[spec[o][3]], spec[o][4]) for o in order]
    return sp, {pos[k]: v for k, v in files.items()}, [decoded[o] for o in order]


@pytest.mark.parametrize("order", [[0, 1, 2, 3, 4, 5, 6], [6, 4, 2, 5, 0, 3, 1], [5, 1, 3, 0, 6, 2, 4]])
def test_fan_out_batch_equals_the_float_batch(torch, fan_out, order):
    import webspeechanalyzer_amd as wsa
    spec, files, decoded = _shuffled(*fan_out, order)
    assert not np.array_equal(fan_out[2][1], fan_out[2][2]) and not np.array_equal(fan_out[2][0], fan_out[2][1])      # the channels differ, and so does the mix
    an = wsa.Analyzer(wsa.Config(output_level=5))
    ns = [c[4] for c in spec]
    ref = an.batch(ns, 16000)
    ref.run_host(decoded, _s(torch))
    want = _tables(ref, torch)
    b = an.batch(ns, 16000)
    fm, ch, sel, src = _args(spec)
    b.run_host_channels([files.get(i) for i in range(len(spec))], fm, ch, sel, src, _s(torch))
    _same_tables(_tables(b, torch), want)
    # every clip with rows of its own: channel 1 is reached, and is not channel 0
    assert len({int(m[0]) for m in want["meta"]}) >= 4
    b.close(); ref.close(); an.close()


def test_resampled_and_mixed_rate_batches_at_level_13(torch):
    import webspeechanalyzer_amd as wsa
    an = wsa.Analyzer(wsa.Config(output_level=13))
    # mixed rates: a stereo 8 kHz A-law call by channel, a 6-channel 44.1 kHz f32 file by its mix and its last channel, a mono 16 kHz i32 clip
    rates = [8000, 8000, 44100, 44100, 16000]
    ns = [int(1.2 * r) for r in rates]
    xa, xb, xc = _speech(torch, 2, ns[0], 8000, 31), _speech(torch, 6, ns[2], 44100, 32), _speech(torch, 1, ns[4], 16000, 33)
    spec = [("alaw", 2, 1, 1, ns[0]), ("alaw", 2, 0, 1, ns[1]), ("f32", 6, MIX, 2, ns[2]), ("f32", 6, 5, 2, ns[3] - 100), ("i32", 1, 0, 4, ns[4])]
    ns[3] -= 100
    files = {1: _file(list(xa), "alaw", 4), 2: _file(list(xb), "f32", 5), 4: _file(list(xc), "i32", 6)}
    decoded = _decoded(spec, files)
    fm, ch, sel, src = _args(spec)
    ref = an.batch(ns, rates, resample_to=16000)
    ref.run_host(decoded, _s(torch))
    want, want_pcm, want_cb = _tables(ref, torch), ref.converted_pcm(_s(torch)), ref.callbacks(_s(torch))
    b = an.batch(ns, rates, resample_to=16000)
    b.run_host_channels([files.get(i) for i in range(len(spec))], fm, ch, sel, src, _s(torch))
    _same_tables(_tables(b, torch), want)
    assert np.array_equal(b.converted_pcm(_s(torch)).view(np.uint32), want_pcm.view(np.uint32))
    assert [c["segments_ci"] for c in b.callbacks(_s(torch))] == [c["segments_ci"] for c in want_cb]
    b.close(); ref.close()
    # one input rate for all clips: a stereo 8 kHz mu-law call, both channels and the mix
    n8 = 9600
    x = _speech(torch, 2, n8, 8000, 34)
    spec = [("mulaw", 2, 0, 0, n8), ("mulaw", 2, 1, 0, n8), ("mulaw", 2, MIX, 0, n8)]
    files = {0: _file(list(x), "mulaw", 7)}
    decoded = _decoded(spec, files)
    fm, ch, sel, src = _args(spec)
    ref = an.batch([n8] * 3, 8000, resample_to=16000)
    ref.run_host(decoded, _s(torch))
    want, want_pcm = _tables(ref, torch), ref.converted_pcm(_s(torch))
    b = an.batch([n8] * 3, 8000, resample_to=16000)
    b.run_host_channels([files[0], None, None], fm, ch, sel, src, _s(torch))
    _same_tables(_tables(b, torch), want)
    assert np.array_equal(b.converted_pcm(_s(torch)).view(np.uint32), want_pcm.view(np.uint32))
    b.close(); ref.close(); an.close()


def test_run_packed_on_planned_channels_inside_a_captured_graph(torch, fan_out):
    import webspeechanalyzer_amd as wsa
    spec, files, decoded = fan_out
    fm, ch, sel, src = _args(spec)
    an = wsa.Analyzer(wsa.Config(output_level=5))
    ns = [c[4] for c in spec]
    b = an.batch(ns, 16000)
    b.enable_timing(False)
    b.set_input_channels(fm, ch, sel, src)
    off = b.packed_offsets()
    assert np.all(off % 16 == 0) and all(off[i] == off[c[3]] for i, c in enumerate(spec)), "a consumer's offset is its source's"
    assert int(off[-1]) == sum((len(f.view(np.uint8)) + 15) // 16 * 16 for f in files.values())

    def image(swap):
        """the files at their offsets, everything else poisoned; swap: the stereo call with its channels exchanged"""
        host = np.full(int(off[-1]), 0xFF, np.uint8)
        for i, f in files.items():
            raw = f.view(np.uint8).reshape(-1)
            if swap and i == 2:
                raw = f.reshape(-1, 2)[:, ::-1].reshape(-1).view(np.uint8)
            host[int(off[i]):int(off[i]) + len(raw)] = raw
        return torch.from_numpy(host)

    swapped = dict(files)
    swapped[2] = files[2].reshape(-1, 2)[:, ::-1].reshape(-1).copy()
    plain = an.batch(ns, 16000)
    refs = []
    for f in (files, swapped):
        plain.run_host(_decoded(spec, f), _s(torch))
        refs.append(_tables(plain, torch))
    assert not np.array_equal(refs[0]["feat"], refs[1]["feat"])
    buf = image(False).cuda()
    assert buf.data_ptr() % 16 == 0
    b.run_packed(buf.data_ptr(), _s(torch))                         # eager first
    _same_tables(_tables(b, torch), refs[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            b.run_packed(buf.data_ptr(), side.cuda_stream)
        for swap, ref in ((True, refs[1]), (False, refs[0])):
            buf.copy_(image(swap))
            g.replay()
            side.synchronize()
            _same_tables(_tables(b, torch), ref)
    # the channel-0 plan takes the batch back, and the channel plan again
    b.set_input_format(fm, ch)
    assert b.packed_offsets()[1] != b.packed_offsets()[2]
    b.set_input_channels(fm, ch, sel, src)
    b.run_packed(buf.data_ptr(), _s(torch))
    _same_tables(_tables(b, torch), refs[0])
    plain.close(); b.close(); an.close()


def test_refusals_name_the_clip_or_stream(torch):
    import webspeechanalyzer_amd as wsa
    an = wsa.Analyzer(wsa.Config(output_level=5))
    b = an.batch([1600, 1600, 1500], 16000)
    clips = [np.zeros(1600 * 65, np.int16)] * 3
    for call in (lambda *a: b.run_host_channels(clips, *a, stream=_s(torch)), lambda *a: b.set_input_channels(*a)):
        with pytest.raises(wsa.WsaError, match="clip 1: select 2 is neither a channel below 2 nor WSA_CHANNEL_MIX"):
            call("i16", [2, 2, 2], [0, 2, "mix"], None)
        with pytest.raises(wsa.WsaError, match=r"clip 2: source 3 outside 0 \.\. 2"):
            call("i16", [2, 2, 2], None, [0, 0, 3])
        with pytest.raises(wsa.WsaError, match=r"clip 2: source 1 is not its own source \(it reads clip 0\)"):
            call("i16", [2, 2, 2], None, [0, 0, 1])
        with pytest.raises(wsa.WsaError, match="clip 0: 1600 frames, its source clip 2 holds 1500"):
            call("i16", [2, 2, 2], None, [2, 1, 2])
        with pytest.raises(wsa.WsaError, match="clip 1: unknown input format 5 "):
            call([1, 5, 1], [2, 2, 2], None, None)
        with pytest.raises(wsa.WsaError, match=r"clip 0: channel count 65 outside 1 \.\. 64"):
            call("i16", [65, 2, 2], None, None)
    assert list(b.packed_offsets()) == [0, 0, 0, 0]                 # nothing was planned by a refused call
    info = capi._BatchInfo()
    an._check(an.L.wsa_batch_get_info(b.h, ctypes.byref(info)))
    assert info.workspace_bytes == b.info["workspace_bytes"]        # ... and nothing allocated: the plan refuses before the staging buffer and the tables
    with pytest.raises(wsa.WsaError, match="before wsa_batch_set_input_format"):
        b.run_packed(16, _s(torch))
    st = an.streams(3, 16000)
    with pytest.raises(wsa.WsaError, match="stream 2: select 2 is neither a channel below 2 nor WSA_CHANNEL_MIX"):
        st.set_input_channels("i16", [2, 9, 9], [0, 1, 2], [0, 0, 0])
    with pytest.raises(wsa.WsaError, match=r"stream 1: source 3 outside 0 \.\. 2"):
        st.set_input_channels("i16", 2, None, [0, 3, 2])
    with pytest.raises(wsa.WsaError, match=r"stream 2: source 1 is not its own source \(it reads stream 0\)"):
        st.set_input_channels("i16", 2, None, [0, 0, 1])
    with pytest.raises(wsa.WsaError, match=r"stream 0: channel count 65 outside 1 \.\. 64"):
        st.set_input_channels("mulaw", [65, 1, 1])
    with pytest.raises(wsa.WsaError, match=r"unknown input format 9 \(WSA_PCM_F32 0, WSA_PCM_I16 1, WSA_PCM_MULAW 2, WSA_PCM_ALAW 3\)"):
        st.set_input_channels("i24", 2)
    with pytest.raises(wsa.WsaError, match="stream 1: source 0 with WSA_PCM_F32"):
        st.set_input_channels("f32", None, None, [0, 0, 2])
    with pytest.raises(wsa.WsaError, match="2 channels with WSA_PCM_F32"):
        st.set_input_channels("f32", 2)
    st.set_input_channels("f32", None, "mix", None)                 # floats: one channel, the mix of one channel is the channel
    st.close(); b.close(); an.close()


# ---- streams

def _steps(wsa, st, fill, n_steps, mixed):
    """n_steps steps, START in the first and STOP in the last; fill(k) writes step k's input -> per step (collect(), converted())"""
    out = []
    for k in range(n_steps):
        ctl = np.full(st.n, wsa.ACTIVE | (wsa.START if k == 0 else 0) | (wsa.STOP if k == n_steps - 1 else 0), np.uint8)
        fill(k)
        st.step_host(ctl, _s_of())
        r = st.collect(_s_of())
        out.append((r, st.converted() if mixed else []))
    return out


def _s_of():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _same_steps(got, want):
    assert len(got) == len(want)
    for k, ((g, gc), (w, wc)) in enumerate(zip(got, want)):
        assert set(g) == set(w)
        for key, val in w.items():
            if key == "tracks":
                continue
            if isinstance(val, np.ndarray):
                assert g[key].shape == val.shape and g[key].tobytes() == val.tobytes(), (k, key)
            else:
                assert g[key] == val, (k, key)
        assert len(gc) == len(wc)
        for i, (a, c) in enumerate(zip(gc, wc)):
            assert a.shape == c.shape and a.tobytes() == c.tobytes(), (k, i, "converted() differs")


@pytest.mark.parametrize("kind", ["plain", "mixed"])
def test_streams_share_packed_rows(torch, kind):
    """a two-channel i16 set: streams 2k and 2k + 1 read row 2k (channel 0 / channel 1); a mu-law set whose streams take the mix of three
    channels.  Three frames per step, four steps, START / STOP, the graph on; against the float set fed the host-decoded rows.  In the mixed
    kind every stream sits at the analysis rate, so converted() is the pull kernel's output itself."""
    import webspeechanalyzer_amd as wsa
    mixed = kind == "mixed"
    fs, n, steps = 16000.0, 6, 4
    an = wsa.Analyzer(wsa.Config(output_level=5))
    make = (lambda k: an.streams(k, [fs] * k, frames_per_step=3, resample_to=fs)) if mixed else (lambda k: an.streams(k, fs, frames_per_step=3))
    for fmt, ch, sel, src in (("i16", 2, [0, 1] * 3, [0, 0, 2, 2, 4, 4]), ("mulaw", 3, ["mix", "mix", 2, "mix", 0, 1], [0, 1, 1, 3, 4, 4])):
        st, twin = make(n), make(n)
        c = st.samples_per_step
        x = _speech(torch, n * ch, steps * c, int(fs), 41)
        rows = {s: _file([x[s * ch + q] for q in range(ch)], fmt, 8 + s).reshape(steps, c * ch) for s in sorted(set(src))}
        st.set_input_channels(fmt, ch, sel, src)
        st.enable_graph(True); twin.enable_graph(True)
        buf, fbuf = st.host_input_packed(), twin.host_input()
        assert buf.dtype == DTYPE[fmt] and buf.shape[1] * buf.itemsize == st.input_stride_bytes

        def fill(k):
            buf[:] = 0x7F7F if fmt == "i16" else 0xFF                # the rows of streams that are no source, and everything behind a row's frames: poison
            for s, r in rows.items():
                buf[s, :c * ch] = r[k]

        def fill_float(k):
            for i in range(n):
                fbuf[i, :c] = capi.pcm_decode(fmt, rows[src[i]][k], ch, sel[i])

        got = _steps(wsa, st, fill, steps, mixed)
        want = _steps(wsa, twin, fill_float, steps, mixed)
        _same_steps(got, want)
        if mixed:
            conv = [np.concatenate([w[1][i] for w in want]) for i in range(n)]
            assert all(len(v) == steps * c for v in conv) and not np.array_equal(conv[0], conv[1]), "streams 0 and 1 take different channels"
        st.close(); twin.close()
    an.close()
