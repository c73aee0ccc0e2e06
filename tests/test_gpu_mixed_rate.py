"""Mixed-rate batches (wsa_batch_create_mixed): every clip of one launch is converted from its own rate by K0 — bit for bit what
oracle/resample.c gives for that rate, a clip already at the analysis rate passing unfiltered — and the whole path on the converted clips
equals the oracle chain resample -> front end -> back end and the per-rate batches of the single-rate entry point."""
import ctypes

import numpy as np
import pytest

from tests.util import callbacks_equal

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

RATES = [8000, 11025, 16000, 22050, 24414, 32000, 44100, 48000, 96000]


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def wsa():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import webspeechanalyzer_amd as w
    return w


def _clips(fs_out, seed0=40):
    """One 2.5 s clip per rate (seeds 40 ... 48), a second clip of another length per rate, and the degenerate lengths 0, 1, 17, 300 on
    four different rates; order shuffled so that the classes interleave.  -> (rates, lens, [n, stride] tensor on the GPU)"""
    from webspeechanalyzer_amd.synth import synth_clips
    items = []
    for k, r in enumerate(RATES):
        items.append((r, int(2.5 * r), seed0 + k))
        items.append((r, int(1.3 * r) + 7 * k + 1, 140 + k))
    for r, n in ((11025, 0), (24414, 1), (fs_out, 17), (96000, 300)):
        items.append((r, n, 200 + n))
    order = np.random.default_rng(7).permutation(len(items))
    items = [items[i] for i in order]
    stride = max(n for _, n, _ in items) + 8
    pcm = torch.zeros((len(items), stride), dtype=torch.float32)
    for c, (r, n, seed) in enumerate(items):
        if n:
            pcm[c, :n] = synth_clips(1, n, fs=r, seed=seed, device="cpu")[0]
    return [float(r) for r, _, _ in items], [n for _, n, _ in items], pcm.cuda().contiguous()


def _check_k0(b, conv, host, rates, lens, fs_out, tag=""):
    from oracle import pyoracle
    refs = []
    for c, (r, n) in enumerate(zip(rates, lens)):
        ref = host[c, :n].copy() if r == fs_out else pyoracle.resample(host[c, :n], r, fs_out)
        assert len(ref) == int(b.n_samples[c]), (tag, c, r, n)
        assert np.array_equal(conv[c, :len(ref)].view(np.uint32), ref.view(np.uint32)), f"{tag} clip {c} ({r} Hz, {n} samples): converted samples differ"
        refs.append(ref)
    return refs


@pytest.mark.parametrize("fs_out", [48000, 16000])
def test_mixed_batch_k0_bit_exact_whole_path_and_per_rate_batches(wsa, fs_out):
    from oracle import pyoracle
    rates, lens, pcm = _clips(fs_out)
    host = pcm.cpu().numpy()
    fe = pyoracle.FrontEnd(pyoracle.fe_cfg(fs=float(fs_out)))
    for level in (5, 13):
        an = wsa.Analyzer(wsa.Config(output_level=level))
        b = an.batch(lens, rates, resample_to=fs_out)
        assert list(b.fs_in) == rates and b.fs == fs_out
        b.run(pcm.data_ptr(), pcm.stride(0), _stream())
        got = b.callbacks(_stream())
        conv = b.converted_pcm(_stream())
        spec, foff = b.spectra(_stream())
        refs = _check_k0(b, conv, host, rates, lens, fs_out, f"level {level}")
        for c, ref in enumerate(refs):
            want = pyoracle.run_backend(fe.run(ref), pyoracle.default_cfg(level=level, bands=fe.bands))
            assert want["segments_ci"] == got[c]["segments_ci"], (level, c)
            ok, why = callbacks_equal(level, want["callbacks"], got[c]["callbacks"], exact=False, tol=1e-4)
            assert ok, (level, c, why)
            if lens[c] >= int(2.5 * rates[c]):
                assert len(want["callbacks"]) > 0, (level, c)
        if level == 5:          # the same clip as a batch of its own: single-rate conversion, or no conversion at all at the analysis rate
            for c, (r, n) in enumerate(zip(rates, lens)):
                one = an.batch([n], fs_out) if r == fs_out else an.batch([n], r, resample_to=fs_out)
                x = pcm[c:c + 1, :max(n, 1)].contiguous()
                one.run(x.data_ptr(), x.stride(0), _stream())
                s1, f1 = one.spectra(_stream())
                assert np.array_equal(s1, spec[foff[c]:foff[c + 1]]), (c, r, n)
                if r != fs_out:
                    c1 = one.converted_pcm(_stream())
                    m = int(b.n_samples[c])
                    assert int(one.n_samples[0]) == m and np.array_equal(c1[0, :m].view(np.uint32), conv[c, :m].view(np.uint32)), (c, r, n)
                one.close()
        b.close(); an.close()


@pytest.mark.parametrize("pad", [0, 1, 2, 3])
def test_mixed_batch_staging_paths_by_clip_alignment(wsa, pad):
    """The four buffer offsets of the single-rate alignment test with a stride that is not a multiple of 4: 16-byte and word staging, every class."""
    from webspeechanalyzer_amd.synth import synth_clips
    rates = [44100.0, 16000.0, 48000.0, 44100.0, 24414.0, 16000.0, 96000.0]
    lens = [3, 5, 4481, 20000 + pad, 33333, 17001, 9999]
    stride = max(lens) + 2 + pad + (1 if (max(lens) + 2 + pad) % 4 == 0 else 0)
    assert stride % 4
    base = synth_clips(1, len(lens) * stride + 8, fs=16000, seed=11 + pad, device="cuda").reshape(-1)
    pcm = base[pad:pad + len(lens) * stride].reshape(len(lens), stride)
    an = wsa.Analyzer(wsa.Config(output_level=5))
    b = an.batch(lens, rates, resample_to=48000)
    b.run(pcm.data_ptr(), pcm.stride(0), _stream())
    b.device_result(_stream())
    _check_k0(b, b.converted_pcm(_stream()), pcm.cpu().numpy(), rates, lens, 48000, f"pad {pad}")
    b.close(); an.close()


def test_mixed_batch_host_entry_points(wsa):
    from webspeechanalyzer_amd.synth import synth_clips
    rates = [16000.0, 44100.0, 48000.0, 22050.0]
    lens = [40000, 100000, 96000, 50000]
    x16 = [(synth_clips(1, n, fs=int(r), seed=60 + i, device="cpu").numpy()[0] * 32767).astype(np.int16) for i, (r, n) in enumerate(zip(rates, lens))]
    floats = [(x.astype(np.float32) / 32768).astype(np.float32) for x in x16]
    stride = max(lens)
    dev = torch.zeros((len(lens), stride), dtype=torch.float32)
    for c, f in enumerate(floats):
        dev[c, :len(f)] = torch.from_numpy(f)
    dev = dev.cuda()
    an = wsa.Analyzer(wsa.Config(output_level=13))
    b = an.batch(lens, rates, resample_to=48000)
    b.run(dev.data_ptr(), dev.stride(0), _stream())
    ref = b.callbacks(_stream())
    assert sum(len(g["callbacks"]) for g in ref) > 0
    b.run_host(floats, _stream())
    got_f = b.callbacks(_stream())
    rng = np.random.default_rng(3)
    chans = [1, 2, 1, 2]
    inter = []
    for x, k in zip(x16, chans):
        m = rng.integers(-30000, 30000, (len(x), k), dtype=np.int16)
        m[:, 0] = x
        inter.append(m.reshape(-1))
    b.run_host_i16(inter, chans, _stream())
    got_i = b.callbacks(_stream())
    for got in (got_f, got_i):
        for c in range(len(lens)):
            assert got[c]["segments_ci"] == ref[c]["segments_ci"], c
            ok, why = callbacks_equal(13, ref[c]["callbacks"], got[c]["callbacks"], exact=False, tol=1e-4)
            assert ok, (c, why)
    b.close(); an.close()


def test_mixed_batch_run_is_graph_capturable(wsa):
    rates, lens, pcm = _clips(48000)
    an = wsa.Analyzer(wsa.Config(output_level=13))
    plain = an.batch(lens, rates, resample_to=48000)
    plain.run(pcm.data_ptr(), pcm.stride(0), _stream())
    ref = plain.rows(_stream())
    assert len(ref["meta"]) > 10
    b = an.batch(lens, rates, resample_to=48000)
    b.enable_timing(False)
    buf = pcm.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        b.run(buf.data_ptr(), buf.stride(0), side.cuda_stream)          # warm (lazy module loads happen outside the capture)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            b.run(buf.data_ptr(), buf.stride(0), side.cuda_stream)
        for _ in range(2):
            buf.zero_(); buf.copy_(pcm)
            g.replay()
            side.synchronize()
            r = b.rows(side.cuda_stream)
            assert np.array_equal(r["meta"], ref["meta"]) and np.array_equal(r["feat"], ref["feat"], equal_nan=True)
    plain.close(); b.close(); an.close()


def test_mixed_batch_refusals_and_many_distinct_rates(wsa):
    an = wsa.Analyzer(wsa.Config(output_level=5))
    for bad in (0.0, -16000.0, 2000.0, 800000.0):
        with pytest.raises(wsa.WsaError, match=r"sample rates.*clip 1"):
            an.batch([1000, 1000, 1000], [16000.0, bad, 44100.0], resample_to=48000)
    h = ctypes.c_void_p()
    ns = np.array([1000, 1000], np.uint32)
    st = an.L.wsa_batch_create_mixed(an.h, 2, ns.ctypes.data, None, 48000.0, ctypes.byref(h))
    assert st == 1 and b"clip" in an.L.wsa_last_error(an.h)
    from webspeechanalyzer_amd.synth import synth_clips
    rates = [16000.0 + 100 * i for i in range(40)]
    lens = [9000 + 37 * i for i in range(40)]
    pcm = synth_clips(40, max(lens) + 4, fs=16000, seed=77, device="cuda")
    b = an.batch(lens, rates, resample_to=48000)
    b.run(pcm.data_ptr(), pcm.stride(0), _stream())
    b.device_result(_stream())
    _check_k0(b, b.converted_pcm(_stream()), pcm.cpu().numpy(), rates, lens, 48000, "40 rates")
    b.close(); an.close()


def test_mixed_batch_one_launch_over_the_whole_list_gives_the_same_samples(wsa, monkeypatch):
    """WSA_RS_ONE_LAUNCH (one launch over the whole work list, the form that lost against one launch per class) converts identically."""
    rates, lens, pcm = _clips(48000)
    out = []
    for one_launch in (False, True):
        if one_launch:
            monkeypatch.setenv("WSA_RS_ONE_LAUNCH", "1")
        an = wsa.Analyzer(wsa.Config(output_level=5))
        b = an.batch(lens, rates, resample_to=48000)
        b.run(pcm.data_ptr(), pcm.stride(0), _stream())
        b.device_result(_stream())
        out.append(b.converted_pcm(_stream()))
        b.close(); an.close()
    monkeypatch.delenv("WSA_RS_ONE_LAUNCH", raising=False)
    assert np.array_equal(out[0].view(np.uint32), out[1].view(np.uint32))
