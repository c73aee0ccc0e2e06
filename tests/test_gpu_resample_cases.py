"""K0 (csrc/resample.hip rs_block, resample_kernel, resample_mixed_kernel) on its own (-m gpu): the hand-built clips of tests/resample_cases.py through the
test entry wsa_debug_resample (capi.debug_resample) against oracle/resample.c, bit for bit.  Per launch: every converted sample equals the oracle's, n_out its
length, the sentinel stands from n_out to the row's end and in the rows of empty clips, and the plan the entry returns {S, J, span, block, LDS bytes, copy} is
the one tests/resample_cases.py works out from no kernel output — which is what says that a case ran on the arm it is named for.  Every launch runs twice, with
zeros and with NaN in all padding (behind n_in inside the row, the whole row of an empty clip, the words in front of the offset base): the kernel loads from
clamped addresses and replaces what lies outside the clip, so the two outputs are the same bits.  tests/test_resample_reference.py (CPU) shows that the cases
notice each one-line fault of the device forms; profiles/resample_k0.md lists nine kernel mutations (the back edge's singles, q_hi, the word path's edge, rows
read once, the chunk loop, the copy run, the blend as one fma, flushed denormals), each built once into a scratch copy of the library, and the test here
that fails on it.

A NaN output is compared as a NaN (sign and payload of a NaN are the device's choice); everything else on bits."""
import numpy as np
import pytest

from tests import resample_cases as rc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENT = 0x7fa5c3d1
NAN_BITS = 0x7fc00000
OFFSETS = (0, 4, 8, 12)
GROUPS = rc.single_rate_groups()
BATCHES = rc.mixed_batches()
_REF = {}


def _gid(g):
    c = g[0]
    return f"{c.fs_in:g}-{c.fs_out:g}" + (f"-S{c.S}" if c.S else "") + (f"-J{c.J}" if c.J else "") + (f"-C{c.C}" if c.C else "") + ("-long" if c.n_out > rc.MAX_OUT else "")


@pytest.fixture(scope="module")
def capi():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from webspeechanalyzer_amd import capi
    return capi


def ref_of(case):
    """(clip, the oracle's conversion): computed once per case, shared by every test, never written to"""
    if case.name not in _REF:
        from oracle import pyoracle
        x = rc.signal(case)
        y = x.copy() if case.fs_in == case.fs_out else pyoracle.resample(x, case.fs_in, case.fs_out)
        x.setflags(write=False); y.setflags(write=False)
        _REF[case.name] = (x, y)
    return _REF[case.name]


def check(res, cases, what, copy_rate=None):
    out = res["out"]
    for i, c in enumerate(cases):
        x, ref = ref_of(c)
        if c.fs_in == c.fs_out and copy_rate is None:            # the single-rate kernel filters also at ratio 1; the copy belongs to the mixed forms
            from oracle import pyoracle
            ref = pyoracle.resample(x, c.fs_in, c.fs_out)
        n = len(ref)
        assert int(res["n_out"][i]) == n == c.n_out, f"{what}, {c}: n_out"
        got = out[i, :n]
        bad = np.nonzero(~((got.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(got) & np.isnan(ref))))[0]
        assert bad.size == 0, f"{what}, {c}: {bad.size} of {n} outputs differ from the oracle, first at {bad[0]}: {got[bad[0]]!r} for {ref[bad[0]]!r}"
        assert np.all(out[i, n:].view(np.uint32) == SENT), f"{what}, {c}: the row behind output {n} was written"
        if c.sig in ("nan", "inf"):
            assert np.array_equal(~np.isfinite(got), rc.nonfinite_expected(c)), f"{what}, {c}: the non-finite outputs are not the windows that hold the sample"


def run_both_paddings(capi, cases, rates, fs_out, what, **kw):
    clips = [ref_of(c)[0] for c in cases]
    stride_in = (max(max(len(x) for x in clips), 1) + 7) & ~3          # rows start 16-byte aligned at offset 0, and every clip has padding behind it
    res = [capi.debug_resample(clips, rates, fs_out, stride_in=stride_in, pad_bits=bits, sentinel=SENT, **kw) for bits in (0, NAN_BITS)]
    assert np.array_equal(res[0]["out"].view(np.uint32), res[1]["out"].view(np.uint32)), f"{what}: NaN in the padding changes the output"
    assert np.array_equal(res[0]["plan"], res[1]["plan"])
    return res[1]


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("group", GROUPS, ids=_gid)
def test_single_rate_kernel(capi, group, offset):
    c0 = group[0]
    res = run_both_paddings(capi, group, c0.fs_in, c0.fs_out, f"form 0 offset {offset}", form=0, S=c0.S, J=c0.J, chunks=c0.C, offset_bytes=offset)
    p = c0.plan
    assert res["plan"].tolist() == [rc.plan_row(p)] and (res["block"], res["lds"]) == (p["block"], p["lds"]), (res["plan"], p)
    check(res, group, f"form 0 offset {offset}")


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("form", (1, 2))
@pytest.mark.parametrize("batch", BATCHES, ids=lambda b: f"to-{b[0].fs_out:g}-{len(b)}-clips")
def test_mixed_kernel(capi, batch, form, offset):
    fs_out = batch[0].fs_out
    res = run_both_paddings(capi, batch, [c.fs_in for c in batch], fs_out, f"form {form} offset {offset}", form=form, offset_bytes=offset)
    rows, max_block, max_lds, _ = rc.mixed_plan(batch)
    assert res["plan"].tolist() == rows and (res["block"], res["lds"]) == (max_block, max_lds)
    check(res, batch, f"form {form} offset {offset}", copy_rate=fs_out)


@pytest.mark.parametrize("name,env", [("rows-S-64-override", {"WSA_RS_S": "64"}), ("J-7-override", {"WSA_RS_J": "7"}),
                                      ("chunks-3-ends-at-c-2", {"WSA_RS_J": "8", "WSA_RS_C": "3"})])
def test_environment_knobs_reach_the_same_code(capi, monkeypatch, name, env):
    """The product route: an.batch(..., resample_to=...) under WSA_RS_S / WSA_RS_J / WSA_RS_C builds its launch through the same resample_shape as the test
    entry; converted_pcm equals the oracle for one case per knob."""
    import webspeechanalyzer_amd as wsa
    case = rc.BY_NAME[name]
    assert {k: int(v) for k, v in env.items()} == {k: v for k, v in (("WSA_RS_S", case.S), ("WSA_RS_J", case.J), ("WSA_RS_C", case.C)) if v}
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    x, ref = ref_of(case)
    pcm = torch.from_numpy(np.array(x)).cuda()[None, :].contiguous()
    s = torch.cuda.current_stream().cuda_stream
    an = wsa.Analyzer(wsa.Config(output_level=5))
    b = an.batch([case.n_in], case.fs_in, resample_to=case.fs_out)
    b.run(pcm.data_ptr(), pcm.stride(0), s)
    b.device_result(s)
    conv = b.converted_pcm(s)
    assert int(b.n_samples[0]) == len(ref) and np.array_equal(conv[0, :len(ref)].view(np.uint32), ref.view(np.uint32)), name
    b.close(); an.close()


@pytest.mark.parametrize("kw", [dict(S=513), dict(S=-1), dict(J=-1), dict(chunks=-1), dict(S=512, J=4096), dict(form=1, S=64), dict(form=2, J=4), dict(offset_bytes=2)],
                         ids=lambda k: "-".join(f"{a}{b}" for a, b in k.items()))
def test_overrides_that_cannot_launch_are_refused(capi, kw):
    """S outside 1 .. 512, J < 1, a staging beyond the device's LDS limit (S = 512, J = 4096: 7.7 MB), overrides on the mixed forms: refused, the output untouched"""
    from webspeechanalyzer_amd import WsaError
    x = ref_of(rc.BY_NAME["n_in-31"])[0]
    with pytest.raises(WsaError, match="error 1"):
        capi.debug_resample([x], 44100.0, 48000.0, **kw)
