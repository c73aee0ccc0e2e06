"""K1 (csrc/fe_r8.hip, fe_rx.hip, fe_r3.hip) on the hand-built geometries and frames of tests/fe_cases.py (-m gpu): Analyzer.batch -> run_frontend ->
spectra against the oracle FE-1 (oracle/frontend.c), which tests/test_fe_reference.py holds against the float64 statement tests/fe_ref.py.  u32 frames,
bit for bit, no tolerance, no case left out.  Every case goes through three arrangements that must give the same bits:
  (a) every clip in a batch of its own, the row exactly as long as the clip and what the case puts behind it;
  (b) all clips of a geometry (same gain and emphasis) in one batch in shuffled order, the row stride 37 samples past the longest clip, NaN in all padding;
  (c) at the two default geometries (16 and 48 kHz) the same signals as a lock-step stream set: the three-frame clips in one step of three frames, the
      first 24 frames of the seam clips four frames per step (frames read back through the test entry wsa_debug_stream_spectra).
Which instantiation a geometry runs is asserted through wsa_debug_fe_choice, and the geometries together with the ones named in LEFT_TO_OTHER_LENGTHS
(reached by test_gpu_parity.py::test_frontend_other_fft_lengths_bit_exact) are all 33 that profiles/frontend_split.md lists.

Run time on an MI355X: 4 s for the file's 25 tests (0.7 s the 16 kHz default geometry with its 33 cases, the slowest).

Mutation check (scratch builds of libwsa, nothing committed; one per device-form fault of tests/fe_ref.py that can be written as a change of arithmetic or
of a select — no address, no count; each ran once; "first" = the first case of the first geometry that failed, frame 1 unless said):
  fault                     change                                                          failed tests   first failure
  padded_tap_multiplies     the commit before the zero word: a padded tap reads a power      5 of 25        16k-default overflow-one-bin alone, band 2: device 0,
                            bin (index clamped to kmax) and multiplies it by its weight 0                  oracle 8419362 (3 bands at 16 kHz, 5 at 48 and 8 kHz)
  flush_denormals           fe_r8 / fe_rx / fe_r3 compiled with -fgpu-flush-denormals-to-zero 4 of 25        16k-default denormal alone, band 1: device 1, oracle 2 (43 values)
  odd_last_sample_dropped   fe_win_select: the `odd` lane takes 0, not the pair's second half 4 of 25        16k-win383 tone-64 alone, band 53: device 9778, oracle 9777
                                                                                                           (the four odd windows: 383, 1151, 1103, 551)
  saturate_at_2_31          to_u32 through v_cvt_i32_f32 and max(., 0)                       5 of 25        16k-default overflow-one-bin alone, band 5: device 2147483647,
                                                                                                           oracle 4294967295
  taps_lo_3                 fe_kernel_r8: the lower band's tap MWL - 1 given weight 0        7 of 25        16k-win258 impulse-126 alone, band 60: device 1437, oracle 1536
  lane0_partner             the k0 == 0 / lane 0 selects of partner_value and                24 of 25       16k-win256 impulse-126 alone, band 56: device 1249, oracle 1564
                            fe_partner_value removed: bin 8R c paired as the other lanes are
  window_by_multiply        fe_win_select: x * (inside ? 1 : 0) instead of the select        0 of 25        EQUIVALENT: the lanes behind the window read the clamped pair
                                                                                                           (win - 2, win - 1), samples of the frame itself; x * 0 is not 0
                                                                                                           only for Inf / NaN, and such a frame is NaN in every bin anyway
                                                                                                           (tests/test_fe_reference.py EQUIVALENT has the measurement)
  emph_index_off_by_one     not built: reading emph[m + 1] moves an address; modelled on the restatement alone (tests/test_fe_reference.py: 16k-win256
                            noise-emphasis)
All failures were comparisons; none faulted.
"""
import re
import os

import numpy as np
import pytest

from tests import fe_cases as fc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# instantiations no geometry of fe_cases selects: other FFT lengths and the larger windows, bit-exact on noise in test_frontend_other_fft_lengths_bit_exact
LEFT_TO_OTHER_LENGTHS = {
    "fe_kernel_r8<4,5,8,true>", "fe_kernel_r8<4,9,12,false>",
    "fe_kernel_rx<2,2,12>", "fe_kernel_rx<4,4,12>", "fe_kernel_rx<16,5,14>", "fe_kernel_rx<16,8,14>", "fe_kernel_rx<16,16,14>", "fe_kernel_rx<32,10,14>",
    "fe_kernel_rx<32,16,14>", "fe_kernel_rx<32,32,14>", "fe_kernel_rx<64,64,14>",
    "fe_kernel_r3<1,2,12>", "fe_kernel_r3<1,3,12>", "fe_kernel_r3<2,3,12>", "fe_kernel_r3<2,6,12>", "fe_kernel_r3<4,5,14>", "fe_kernel_r3<4,8,14>",
    "fe_kernel_r3<4,12,14>", "fe_kernel_r3<8,10,14>", "fe_kernel_r3<8,24,14>", "fe_kernel_r3<16,20,14>", "fe_kernel_r3<16,32,14>", "fe_kernel_r3<16,48,14>",
    "fe_kernel_r3<32,96,14>",
}


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def wsa():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import webspeechanalyzer_amd as w
    return w


def _groups(gname):
    """the geometry's cases by (gain, emphasis): one analyzer each"""
    out = {}
    for c in fc.cases(gname):
        out.setdefault(c.key, []).append(c)
    return out


def _run(an, g, group, order, stride, pad):
    """one batch of the cases `order` picks: rows of `stride` samples, the clip, what the case puts behind it, then `pad`; the cases' frames in case order"""
    rows = np.full((len(order), stride), pad, np.float32)
    for i, k in enumerate(order):
        c = group[k]
        rows[i, :len(c.clip)] = c.clip
        rows[i, len(c.clip):len(c.clip) + len(c.tail)] = c.tail
    b = an.batch([len(group[k].clip) for k in order], g.fs)
    dev = torch.from_numpy(rows).cuda()
    b.run_frontend(dev.data_ptr(), dev.stride(0), _stream())
    spec, foff = b.spectra(_stream())
    b.close()
    return {k: spec[foff[i]:foff[i + 1]].copy() for i, k in enumerate(order)}


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        f, m = np.argwhere(got != want)[0]
        raise AssertionError(f"{what}: {(got != want).sum()} of {got.size} values differ; first frame {f} band {m}: device {got[f, m]} oracle {want[f, m]}")


@pytest.mark.parametrize("gname", [g.name for g in fc.GEOMETRIES])
def test_hand_built_frames_equal_the_oracle_in_every_arrangement(wsa, gname):
    from webspeechanalyzer_amd import capi
    g = fc.BY_NAME[gname]
    for key, group in _groups(gname).items():
        an = wsa.Analyzer(wsa.Config(**g.config_kw(*key)))
        assert capi.debug_fe_choice(an, g.fs) == g.inst
        geo, fe = an.geometry(g.fs), g.oracle(*key)
        assert (geo["nfft"], geo["win"], geo["hop"], geo["bands"], geo["kmax"]) == (fe.nfft, fe.win, fe.hop, fe.bands, fe.kmax)
        want = [fc.expected(c) for c in group]
        by_name = {c.name: k for k, c in enumerate(group)}
        # (a) every clip alone
        alone = {}
        for k, c in enumerate(group):
            alone[k] = _run(an, g, group, [k], len(c.clip) + len(c.tail), 0.0)[k]
            _same(alone[k], want[k], f"{gname} {key} case {c.name} alone")
        # (b) all together, shuffled, NaN in all padding
        order = [int(k) for k in np.random.default_rng(len(group)).permutation(len(group))]
        stride = max(len(c.clip) for c in group) + 37
        together = _run(an, g, group, order, stride, np.nan)
        for k, c in enumerate(group):
            _same(together[k], want[k], f"{gname} {key} case {c.name} in the shuffled batch")
            assert np.array_equal(together[k], alone[k])
            if c.same_as:
                _same(together[k], together[by_name[c.same_as]], f"{gname} case {c.name} against {c.same_as}")
        an.close()


@pytest.mark.parametrize("gname", fc.DEFAULTS)
def test_the_same_signals_as_streams(wsa, gname):
    from webspeechanalyzer_amd import capi
    g = fc.BY_NAME[gname]
    for key, group in _groups(gname).items():
        fe = g.oracle(*key)
        kw = dict(g.config_kw(*key), output_level=5)
        short = [c for c in group if len(c.clip) == fe.win + 2 * fe.hop]
        seams = [c for c in group if c.name.startswith("seam-")]
        for cases_, F, frames in ((short, 3, 3), (seams, 4, 24)):
            if not cases_:
                continue
            an = wsa.Analyzer(wsa.Config(**kw))
            st = an.streams(len(cases_), g.fs, frames_per_step=F)
            sps = st.samples_per_step
            assert sps == F * fe.hop and fe.hop == fe.win
            got = []
            for s in range(frames // F):
                ctl = np.full(len(cases_), wsa.ACTIVE | (wsa.START if s == 0 else 0) | (wsa.STOP if s == frames // F - 1 else 0), np.uint8)
                buf = torch.from_numpy(np.stack([c.clip[s * sps:(s + 1) * sps] for c in cases_])).cuda()
                st.step(buf.data_ptr(), buf.stride(0), ctl, _stream())
                st.collect(_stream())
                got.append(capi.debug_stream_spectra(st, fe.bands))
            got = np.concatenate(got, axis=1)
            for i, c in enumerate(cases_):
                _same(got[i], fc.expected(c)[:frames], f"{gname} {key} case {c.name} as a stream, {F} frames per step")
            st.close(); an.close()


def test_the_geometries_name_their_instantiations_and_the_table_is_covered():
    table = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "frontend_split.md")).read()
    table = table[table.index("| instantiation | reached by"):table.index("## Suites")]
    listed = {re.sub(r"\s", "", n) for n in re.findall(r"^\| `(fe_kernel_\w+<[^>]*>)`", table, re.M)}
    assert len(listed) == 33
    here = {g.inst for g in fc.GEOMETRIES}
    assert here <= listed and LEFT_TO_OTHER_LENGTHS <= listed
    assert here | LEFT_TO_OTHER_LENGTHS == listed and not here & LEFT_TO_OTHER_LENGTHS
