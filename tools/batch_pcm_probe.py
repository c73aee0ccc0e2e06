#!/usr/bin/env python3
"""Time of one batch from page-locked host memory per clip encoding (spec PK-2; profiles/batch_pcm.md), and the unpack kernel's own time.

  step host     1024 clips x 10 s at 16 kHz in wsa_host_alloc slabs, clips back to back.  Cases, alternating round by round inside one process:
                f32 (wsa_batch_run_host), i16_old (wsa_batch_run_host_i16), i16 / mulaw / i24 / f32_packed (wsa_batch_run_host_packed).
                Wall time from the call to the result counters on the host (wsa_batch_result), median and spread over the rounds.  The two
                entries that exist without PK-2 are unchanged by it: their rows are the parent's numbers, taken in the same session.
  step unpack   the same clips device-resident: wsa_batch_run_packed per format beside wsa_batch_run on the decoded floats, device events
                around each; the difference of the medians is batch_unpack_kernel's time (one kernel in front of an unchanged run).
  step channels the interleaved path (spec PK-3; profiles/pcm_channels.md): the same clips as stereo files, i16 and i24, device-resident, the second
                channel another signal.  Per format: channel 0 through batch_unpack_kernel (wsa_batch_set_input_format, the strided path), then
                batch_deinterleave_kernel (wsa_batch_set_input_channels) for channel 0 alone, for both channels (2 x clips analyses) and for both
                channels and the mix (3 x clips analyses) — each beside wsa_batch_run on the decoded floats of the same analyses, device events
                around each, the difference of the medians the kernel's time; and the bytes each kernel has to move.

Run without --step, the script touches no GPU itself: it starts every step as a child under its own time limit and stops at the first
that fails.

    python tools/batch_pcm_probe.py [--clips 1024] [--seconds 10] [--rounds 15] [--only STEP] [--out FILE]"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--clips", type=int, default=1024)
ap.add_argument("--seconds", type=float, default=10.0)
ap.add_argument("--rounds", type=int, default=15)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--step", default="", help="host | unpack | channels (a child of the driver)")
ap.add_argument("--only", default="", help="the driver runs this step alone")
ap.add_argument("--limit", type=int, default=240, help="seconds a step may take")
ap.add_argument("--out", default="")
args = ap.parse_args()
FS = 16000
STEPS = ["host", "unpack", "channels"]

if not args.step:
    results = []
    for step in ([args.only] if args.only else STEPS):       # each GPU step under its own limit, chained: a failure ends the probe
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--step", step, "--clips", str(args.clips),
               "--seconds", str(args.seconds), "--rounds", str(args.rounds), "--warmup", str(args.warmup)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:
            print(json.dumps(dict(step=step, failed=r.returncode)), flush=True)
            sys.exit(r.returncode)
        results += [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    if args.out:
        json.dump(results, open(args.out, "w"), indent=1)
    sys.exit(0)

import numpy as np
import torch

import webspeechanalyzer_amd as wsa
from webspeechanalyzer_amd import capi
from webspeechanalyzer_amd.synth import synth_clips

n, ns = args.clips, int(args.seconds * FS)
an = wsa.Analyzer(wsa.Config(output_level=5))
L = capi.lib()
stream = torch.cuda.current_stream().cuda_stream
distinct = min(n, 32)                        # distinct signals, repeated over the batch: the link does not care, the kernels hardly
x = synth_clips(distinct, ns, fs=FS, seed=5, device="cuda").cpu().numpy().astype(np.float64)


def mulaw_encode(v):
    table = (capi.pcm_decode("mulaw", np.arange(256, dtype=np.uint8)).astype(np.float64) * 32768).astype(np.int64)
    order = np.argsort(table, kind="stable")
    srt = table[order]
    q = np.clip(np.rint(v * 32767.0), -32768, 32767).astype(np.int64)
    hi = np.clip(np.searchsorted(srt, q), 1, 255)
    return order[np.where(np.abs(srt[hi] - q) < np.abs(srt[hi - 1] - q), hi, hi - 1)].astype(np.uint8)


def encoded(fmt):
    """[distinct, bytes per clip] uint8"""
    if fmt == "f32":
        return x.astype("<f4").view(np.uint8).reshape(distinct, -1)
    if fmt == "i16":
        return np.clip(np.rint(x * 32767.0), -32768, 32767).astype("<i2").view(np.uint8).reshape(distinct, -1)
    if fmt == "mulaw":
        return mulaw_encode(x).reshape(distinct, -1)
    q = np.rint(x * 8388607.0).astype(np.int64) & 0xFFFFFF           # i24
    return np.stack([q & 0xFF, (q >> 8) & 0xFF, q >> 16], axis=-1).astype(np.uint8).reshape(distinct, -1)


slabs = []


def pinned_clips(fmt):
    """the batch's clips in one page-locked slab, back to back: [n, bytes per clip] uint8 view"""
    e = encoded(fmt)
    p = ctypes.c_void_p()
    assert L.wsa_host_alloc(an.h, n * e.shape[1], ctypes.byref(p)) == 0
    slabs.append(p)
    view = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)), shape=(n, e.shape[1]))
    for i in range(n):
        view[i] = e[i % distinct]
    return view


def stats(name, ms, **kw):
    ms = np.asarray(ms)
    r = dict(case=name, clips=n, seconds=args.seconds, rounds=int(ms.size), median_ms=float(np.median(ms)), min_ms=float(ms.min()), max_ms=float(ms.max()),
             p25_ms=float(np.percentile(ms, 25)), p75_ms=float(np.percentile(ms, 75)), **kw)
    print(json.dumps(r), flush=True)


DT = {"f32": np.float32, "i16": np.int16, "mulaw": np.uint8, "i24": np.uint8}
BYTES = {"f32": 4, "i16": 2, "mulaw": 1, "i24": 3}

if args.step == "host":
    data = {f: pinned_clips(f) for f in ("f32", "i16", "mulaw", "i24")}
    # the C entries themselves, on pointer tables built once: the wrapper's per-clip checks are no part of what is compared
    ptrs = {f: (ctypes.c_void_p * n)(*[data[f][i].ctypes.data for i in range(n)]) for f in data}
    fmts = {f: (ctypes.c_int32 * n)(*[capi.pcm_format(f)] * n) for f in data}
    packed = lambda f: (lambda b: L.wsa_batch_run_host_packed(b.h, ptrs[f], fmts[f], None, stream))
    cases = [("f32", "f32", lambda b: L.wsa_batch_run_host(b.h, ptrs["f32"], stream)), ("i16_old", "i16", lambda b: L.wsa_batch_run_host_i16(b.h, ptrs["i16"], None, stream)),
             ("i16", "i16", packed("i16")), ("mulaw", "mulaw", packed("mulaw")), ("i24", "i24", packed("i24")), ("f32_packed", "f32", packed("f32"))]
    opened = []
    for name, fmt, call in cases:
        b = an.batch([ns] * n, FS)
        b.enable_timing(False)
        opened.append((name, fmt, call, b))
    ms = {name: [] for name, *_ in cases}
    rows = {}
    for r in range(args.warmup + args.rounds):
        for name, fmt, call, b in opened:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            an._check(call(b))
            res = b.device_result(stream)
            t1 = time.perf_counter()
            rows[name] = int(res.n_rows)
            if r >= args.warmup:
                ms[name].append((t1 - t0) * 1e3)
    for name, fmt, call, b in opened:
        stats(name, ms[name], step="host", format=fmt, link_bytes=int(n * ns * BYTES[fmt]), rows=rows[name])
        b.close()
elif args.step in ("unpack", "channels"):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(call):
        out = []
        for r in range(args.warmup + args.rounds):
            torch.cuda.synchronize()
            ev0.record()
            call()
            ev1.record()
            ev1.synchronize()
            if r >= args.warmup:
                out.append(ev0.elapsed_time(ev1))
        return out

    for fmt in (("i16", "i24") if args.step == "channels" else ()):
        sb = BYTES[fmt]
        mono = encoded(fmt).reshape(distinct, ns, sb)
        e = np.stack([mono, np.roll(mono, 1, axis=0)], axis=2).reshape(distinct, -1)      # stereo files: channel 1 is the next signal
        flo = {sel: np.stack([capi.pcm_decode(fmt, e[i].view(DT[fmt]), 2, sel) for i in range(distinct)]) for sel in (0, 1, "mix")}
        file_bytes = n * ns * 2 * sb
        # (name, select per analysis of a file, the plan): the analyses of file i stand side by side, the first is the source
        for name, sels in (("ch0_strided", None), ("ch0", [0]), ("both", [0, 1]), ("both_mix", [0, 1, "mix"])):
            k = len(sels) if sels else 1
            b = an.batch([ns] * (n * k), FS)
            b.enable_timing(False)
            if sels is None:
                b.set_input_format(fmt, [2] * n)
            else:
                b.set_input_channels(fmt, [2] * (n * k), sels * n, [i - i % k for i in range(n * k)])
            off = b.packed_offsets()
            host = np.zeros(int(off[-1]), np.uint8)
            for i in range(n):
                host[int(off[i * k]):int(off[i * k]) + e.shape[1]] = e[i % distinct]
            dev = torch.from_numpy(host).cuda()
            floats = torch.from_numpy(np.stack([flo[sel][i % distinct] for i in range(n) for sel in (sels or [0])])).cuda().contiguous()
            t_packed = timed(lambda: b.run_packed(dev.data_ptr(), stream))
            t_float = timed(lambda: b.run(floats.data_ptr(), floats.stride(0), stream))
            # read: the strided path touches every 64-byte line of a stereo file for half of its content; the tile reads each byte once
            stats("channels_%s_%s" % (fmt, name), t_packed, step="channels", format=fmt, analyses=n * k, float_run_median_ms=float(np.median(t_float)),
                  kernel_ms=float(np.median(t_packed) - np.median(t_float)), source_bytes=int(file_bytes), bytes_used=int(file_bytes if sels else file_bytes // 2),
                  bytes_written=int(n * k * ns * 4))
            b.close()
            del dev, floats
    for fmt in (("f32", "i16", "mulaw", "i24") if args.step == "unpack" else ()):
        e = encoded(fmt)
        b = an.batch([ns] * n, FS)
        b.enable_timing(False)
        b.set_input_format(fmt)
        off = b.packed_offsets()
        host = np.zeros(int(off[-1]), np.uint8)
        for i in range(n):
            host[int(off[i]):int(off[i]) + e.shape[1]] = e[i % distinct]
        dev = torch.from_numpy(host).cuda()
        floats = torch.from_numpy(np.stack([capi.pcm_decode(fmt, e[i % distinct].view(DT[fmt])) for i in range(distinct)])).cuda()
        floats = floats.repeat((n + distinct - 1) // distinct, 1)[:n].contiguous()
        t_packed = timed(lambda: b.run_packed(dev.data_ptr(), stream))
        t_float = timed(lambda: b.run(floats.data_ptr(), floats.stride(0), stream))
        stats("unpack_" + fmt, t_packed, step="unpack", format=fmt, float_run_median_ms=float(np.median(t_float)),
              unpack_ms=float(np.median(t_packed) - np.median(t_float)), packed_bytes=int(off[-1]))
        b.close()
        del dev, floats
for p in slabs:
    L.wsa_host_free(p)
an.close()
