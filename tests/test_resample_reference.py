"""The batch rate converter's test infrastructure, on the CPU: the restatement of the device forms (tests/resample_ref.py) against oracle/resample.c, its
one-line faults against the hand-built cases (tests/resample_cases.py), the oracle against an independent long-double evaluation of RS-1, and the geometry
model's plan against the table of stride classes.  `pytest -s` prints the arm table and the case that catches each fault.
tests/test_gpu_resample_cases.py holds the kernels to the same oracle on the same cases."""
import numpy as np
import pytest

from tests import resample_cases as rc
from tests import resample_ref as rr

SENT = 0x7fa5c3d1          # a NaN no arithmetic produces: the untouched rest of an output row


@pytest.fixture(scope="module")
def oracle():
    from oracle import pyoracle
    cache = {}

    def run(case):
        if case.name not in cache:
            x = rc.signal(case)
            cache[case.name] = (x, x.copy() if case.fs_in == case.fs_out else pyoracle.resample(x, case.fs_in, case.fs_out))
        return cache[case.name]
    return run


def same(a, b):
    """bit for bit, any NaN equal to any NaN (a NaN's sign and payload are the host's or the device's choice, not RS-1's)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def _forms(case, x, faults=(), aligned=True):
    stride = case.n_out + case.plan["S"] * case.plan["J"] + 8 if case.fs_in != case.fs_out else case.n_out + 8
    return rr.device_forms(case, x, stride, SENT, aligned=aligned, faults=faults, copy=case.fs_in == case.fs_out)


def test_arm_table_is_complete():
    t = rc.check_cases()
    print("\narm" + " " * 41 + "count  first case")
    for a in sorted(t):
        print(f"{a:44s}{t[a][0]:5d}  {t[a][1]}")
    for a, why in rc.UNREACHABLE.items():
        print(f"{a:44s}    -  unreachable: {why}")
    print(f"{'rows:S%L==0:rounding-reload':44s}    -  " + ", ".join(f"{fs} -> 48000: {'none below 2^20 outputs' if c is None else c.name}" for fs, c in rc.ROUNDING.items()))
    for a in rc.REQUIRED + rc.REQUIRED_MIXED:
        assert t[a][0] > 0, a


def test_restatement_equals_the_oracle_on_every_case(oracle):
    for case in rc.CASES:
        x, ref = oracle(case)
        for aligned in (True, False):
            got, n_out = _forms(case, x, aligned=aligned)
            assert n_out == len(ref), case
            assert same(got[:n_out], ref), f"{case} (aligned {aligned}): the restatement differs from oracle/resample.c"
            assert np.all(got[n_out:].view(np.uint32) == SENT), case


def test_nonfinite_outputs_are_exactly_the_windows_that_hold_the_sample(oracle):
    n = 0
    for case in rc.CASES:
        if case.sig in ("nan", "inf"):
            _, ref = oracle(case)
            want = rc.nonfinite_expected(case)
            assert np.array_equal(~np.isfinite(ref), want) and want.any() and not want.all(), case
            n += 1
    assert n == 4


# fault -> cases named for the arm the fault sits on; the first one must notice it
CATCHES = {
    "back-edge-last-dropped": ["back-e0-last-run", "back-e1-first-run", "back-e2-middle-run"],
    "q_hi-one-short": ["back-e3-last-run", "back-e0-first-run", "back-e1-middle-run"],
    "rows-not-reloaded": ["rows-S-64-override", "rows-S-100-override", "period-47999-least-slack", "non-integer-rate-44100.5"],
    "window-start-rounded": ["window-start-lo-lo4-1", "window-start-lo-lo4-0"],
    "break-left-out": ["last-run-1-outputs", "last-run-S-1-outputs"],
    "subnormals-flushed": ["signal-sub-44100", "signal-subimp-44100", "signal-sub-48000-16000"],
    "blend-one-fma": ["signal-cancel-blend-roundings"],
    "taps-descending": ["rows-no-reload-44100"],
    "span-4-short": ["period-47999-least-slack"],
    "chunks-first-run-only": ["chunks-2-ends-at-c-1", "chunks-3-ends-at-c-2"],
    "copy-run-off-by-one": ["copy-8192", "copy-8193", "copy-16385"],
}


def test_every_fault_changes_a_case_named_for_its_arm(oracle):
    assert set(CATCHES) | set(rr.EQUIVALENT) == set(rr.FAULTS)
    lines = []
    for fault, names in CATCHES.items():
        caught = []
        for name in names:
            case = rc.BY_NAME[name]
            x, ref = oracle(case)
            got, n_out = _forms(case, x, faults=[fault])
            if not (same(got[:n_out], ref) and np.all(got[n_out:].view(np.uint32) == SENT)):
                caught.append(name)
        assert caught and caught[0] == names[0], f"fault {fault}: {names[0]} does not notice it (noticed by {caught})"
        lines.append(f"{fault:28s} {', '.join(caught)}")
    for fault in rr.EQUIVALENT:                                   # no input can tell these from the kernel: the model's reasons, and no case changes
        for case in rc.CASES:
            if case.n_out <= 5000:
                x, ref = oracle(case)
                got, n_out = _forms(case, x, faults=[fault])
                assert same(got[:n_out], ref), (fault, case)
        lines.append(f"{fault:28s} equivalent: {rr.FAULTS[fault]}")
    print("\nfault" + " " * 24 + "caught by")
    print("\n".join(lines))


def test_oracle_within_the_running_error_bound_of_the_long_double_evaluation(oracle):
    worst = 0.0
    for case in rc.CASES:
        if case.fs_in == case.fs_out or case.sig in ("nan", "inf", "big") or case.n_out == 0:
            continue
        x, ref = oracle(case)
        hp, mag = rr.rs1_longdouble(x, case.fs_in, case.fs_out)
        err, bound = np.abs(ref.astype(np.longdouble) - hp), rr.error_bound(hp, mag)
        k = int(np.argmax(err - bound))
        assert err[k] <= bound[k], f"{case}: output {k} is {float(err[k]):.3e} from the long-double value, bound {float(bound[k]):.3e}"
        worst = max(worst, float(np.max(err / bound)))
    assert 0 < worst <= 1.0


def test_model_plan_equals_the_stride_table():
    for fs_in, fs_out, S, block in rc.STRIDE_TABLE:
        p = rc.plan(fs_in, fs_out)
        assert (p["S"], p["block"]) == (S, block), (fs_in, fs_out, p)
        assert p["J"] == rc.rs_j(S, fs_in / fs_out) and p["lds"] == rc.TABLE_BYTES + 4 * rc.rs_xlen(p["span"]) <= 65536
    assert rc.resample_stride(rc.FS_300, 48000) == (300, "search") and rc.resample_stride(rc.FS_400, 48000) == (400, "search")
    assert rc.plan(128000, 8000)["J"] == 1 and rc.plan(48000, 3000)["J"] == 1 and rc.plan(3000, 48000)["J"] == 96
    assert rc.plan(44100.5, 48000)["S"] == 256 and rc.plan(47999, 48000)["S"] == 256 and rc.plan(11025, 48000)["S"] == 256


def test_rounding_never_moves_an_output_to_another_row_below_2_20_outputs():
    """With S a multiple of the period a lane re-reads its rows only where the fp64 product n * ratio lands on another row than the period's: the model finds
    no such output below 2^20 at any rate pair of the stride table (nor at the two pairs of the search), so that arm has no case; rows are re-read in the
    cases with S no multiple of the period, a long period or a non-integer rate."""
    for fs_in, fs_out in [(a, b) for a, b, _, _ in rc.STRIDE_TABLE] + [(16000, 48000), (rc.FS_300, 48000), (rc.FS_400, 48000)]:
        assert rc._first_rounding_reload(fs_in, fs_out) is None, (fs_in, fs_out)
    assert rc.ROUNDING == {44100: None, 16000: None} and "rows:S%L==0:rounding-reload" not in rc.REQUIRED
    assert sum(rc.geometry(rc.BY_NAME[n])["reloads"] > 0 for n in ("rows-S-64-override", "rows-S-100-override", "period-47999-least-slack", "period-640-11025",
                                                                   "period-8000-24414", "non-integer-rate-44100.5")) == 6


def test_staged_length_covers_every_run_start():
    """The default staging bound on record: over 18 rate pairs and 200 000 run starts each, the last output's window ends inside rs_xlen(span); the least slack
    is 2 samples (47999 -> 48000) and at 24414 -> 48000 the need exceeds span by one sample, which only rs_xlen's rounding covers."""
    pairs = [(44100, 48000), (16000, 48000), (8000, 48000), (22050, 48000), (32000, 48000), (48000, 16000), (44100, 16000), (96000, 48000), (11025, 44100),
             (128000, 8000), (3000, 48000), (48000, 44100), (16000, 44100), (24414, 48000), (47999, 48000), (11025, 48000), (44100.5, 48000), (42336, 48000)]
    least, over = 10**9, {}
    for fs_in, fs_out in pairs:
        p = rc.plan(fs_in, fs_out)
        SJ = p["S"] * p["J"]
        n0 = np.arange(200000, dtype=np.float64) * SJ
        lo = np.floor(n0 * p["ratio"]).astype(np.int64) - 16
        lo4 = lo & ~3
        need = np.trunc((n0 + (SJ - 1)) * p["ratio"] - (lo4 + 16).astype(np.float64)).astype(np.int64) + 32
        xlen = rc.rs_xlen(p["span"])
        assert need.max() <= xlen, (fs_in, fs_out, int(need.max()), xlen)
        least = min(least, xlen - int(need.max()))
        over[(fs_in, fs_out)] = int(need.max()) - p["span"]
    assert least == 2 and over[(47999, 48000)] + 2 == rc.rs_xlen(rc.plan(47999, 48000)["span"]) - rc.plan(47999, 48000)["span"]
    assert over[(24414, 48000)] == 1 and max(over.values()) == 1
