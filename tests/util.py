"""Shared helpers for the parity tests."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def jsnum(x):
    """ref_driver.js writes non-finite Numbers as strings ("NaN", "Infinity", "-Infinity")."""
    return float(x) if isinstance(x, str) else x


def jsvec(v):
    return np.array([jsnum(x) for x in v], dtype=np.float64)


def same_f64(a, b):
    """bitwise-equal doubles, NaN == NaN."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def rel_err(a, b, abs_floor=1e-6):
    """max relative error with an absolute floor; NaN/Inf positions must coincide."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return np.inf
    fin = np.isfinite(a) & np.isfinite(b)
    if not bool(((a == b) | (np.isnan(a) & np.isnan(b)))[~fin].all()):
        return np.inf
    if not fin.any():
        return 0.0
    return float(np.max(np.abs(a[fin] - b[fin]) / np.maximum(np.abs(b[fin]), abs_floor)))


def load_backend_golden():
    # the spectra are split over two files (each under the size limit for a committed file)
    spectra = {}
    for f in ("backend_spectra.npz", "backend_spectra_2.npz"):
        spectra.update(np.load(os.path.join(GOLDEN, f)))
    cases = json.load(open(os.path.join(GOLDEN, "backend_expected.json")))["cases"]
    return spectra, cases


def callbacks_equal(level, ref_cbs, got_cbs, exact=True, tol=1e-4):
    """Compare the callback sequences (reference JSON form vs ours).  Indices / timestamps always
    exact; feature vectors bit-exact (exact=True) or within tol relative error."""
    if len(ref_cbs) != len(got_cbs):
        return False, f"callback count {len(ref_cbs)} != {len(got_cbs)}"
    for r, o in zip(ref_cbs, got_cbs):
        if r[0] != o[0]:
            return False, f"si {r[0]} != {o[0]}"
        if level == 3:                 # (si, label, tracks): integers and exact doubles only (velocities are k/2, k/3)
            if json.loads(json.dumps(r[2])) != json.loads(json.dumps(o[2])):
                return False, f"si {r[0]} ranked tracks differ"
        elif level == 12:
            if [list(x) for x in r[2]] != [list(x) for x in o[2]]:
                return False, f"si {r[0]} syllable times {r[2]} != {o[2]}"
            if len(r[3]) != len(o[3]):
                return False, f"si {r[0]} row count {len(r[3])} != {len(o[3])}"
            for a, b in zip(r[3], o[3]):
                ok = same_f64(jsvec(a), b) if exact else rel_err(b, jsvec(a)) <= tol
                if not ok:
                    return False, f"si {r[0]} polynomial rows differ"
        elif level == 5:
            if not same_f64(jsvec(r[2]), o[2]):
                return False, f"si {r[0]} time {r[2]} != {list(o[2])}"
            ok = same_f64(jsvec(r[3]), o[3]) if exact else rel_err(o[3], jsvec(r[3])) <= tol
            if not ok:
                return False, f"si {r[0]} features differ"
        elif level == 13:
            if [list(x) for x in r[2]] != [list(x) for x in o[2]]:
                return False, f"si {r[0]} syllable times {r[2]} != {o[2]}"
            if len(r[3]) != len(o[3]):
                return False, f"si {r[0]} syllable count"
            for a, b in zip(r[3], o[3]):
                ok = same_f64(jsvec(a), b) if exact else rel_err(b, jsvec(a)) <= tol
                if not ok:
                    return False, f"si {r[0]} syllable features differ"
        elif level == 11:
            if not same_f64(jsvec(r[2]), o[2]):
                return False, f"callback time {r[2]} != {list(o[2])}"
            ok = same_f64(jsvec(r[3]), o[3]) if exact else rel_err(o[3], jsvec(r[3])) <= tol
            if not ok:
                return False, "utterance features differ"
        elif level == 10:
            if [list(x) for x in r[2]] != [list(x) for x in o[2]]:
                return False, f"si {r[0]} syllable times {r[2]} != {o[2]}"
            if len(r[3]) != len(o[3]):
                return False, f"si {r[0]} syllable count"
            for a, b in zip(r[3], o[3]):
                ra = np.array([[jsnum(x) for x in row] for row in a], dtype=np.float64).reshape(-1, 9)
                if not same_f64(ra, np.asarray(b, dtype=np.float64).reshape(-1, 9)):
                    return False, f"si {r[0]} syllable formant frames differ"
        elif level == 4:
            if not same_f64(jsvec(r[2]), o[2]):
                return False, f"si {r[0]} time"
            a = np.array([[jsnum(x) for x in row] for row in r[3]], dtype=np.float64)
            if not same_f64(a, np.asarray(o[3], dtype=np.float64)):
                return False, f"si {r[0]} formant frames differ"
    return True, ""


def feature_events(fr9):
    """Energy events per formant column of [n, 9] straightened frames: the peak-then-halve walk of the reference's formant_features
    (ref dist/main.js:2 @B32369), counts only."""
    counts = []
    for n in range(3):
        prev, S, L, c = False, 0, 0.0, 0
        for r, E in zip(np.asarray(fr9)[:, 3 * n].tolist(), np.asarray(fr9)[:, 3 * n + 1].tolist()):
            if r > 0 and E > 0:
                if prev:
                    if E > L:
                        L, S = E, 1
                    elif S == 1 and E < L / 2:
                        c += 1 if L > 10 else 0
                        L, S = 0.0, -1
                prev = True
            else:
                prev, S, L = False, 0, 0.0
        counts.append(c)
    return counts


def long_voiced_audio(seconds=26.0, fs=16000):
    """Three frequency-wobbled sines at 420 / 1150 / 2300 Hz without a pause, the amplitude down to 0.15 - 0.4 of itself for 30 - 60 ms every 0.37 s (an
    energy event of formant_features each), 0.1 s of silence at both ends: one voiced span as long as the clip."""
    rng = np.random.default_rng(2600)
    n = int(seconds * fs)
    t = np.arange(n) / fs
    env = np.ones(n)
    for a in np.arange(0.5, seconds - 0.3, 0.37):
        i = int(a * fs)
        env[i:i + int(rng.uniform(0.03, 0.06) * fs)] *= rng.uniform(0.15, 0.4)
    sig = np.zeros(n)
    for j, (f0, amp) in enumerate(((420.0, 0.3), (1150.0, 0.2), (2300.0, 0.12))):
        phase = 2 * np.pi * np.cumsum(f0 * (1 + 0.02 * np.sin(2 * np.pi * t / (0.9 + 0.17 * j)))) / fs
        sig += amp * np.sin(phase)
    sig *= env
    lead = int(0.1 * fs)
    sig[:lead] = 0; sig[n - lead:] = 0
    return sig.astype(np.float32)
