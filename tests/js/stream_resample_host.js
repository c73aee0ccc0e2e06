// stream_resample_host.js — drives js/formantanalyzer.js's StreamOpen over sources of different rates for tests/test_js_host_stream_resample.py.
// usage: node stream_resample_host.js job.json  -> JSON on stdout
//   job = {clips: [{pcm: f32 file, fs}], settings, model | null, frames_per_step}
//   out = {stream: {callbacks per source, preds, handle}, batch: {callbacks per clip, preds}}
'use strict';
const fs = require('fs');
const path = require('path');
const fa = require(path.join(__dirname, '..', '..', 'webspeechanalyzer_amd', 'js', 'formantanalyzer.js'));

const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const num = (x) => (Number.isFinite(x) ? x : String(x));
const vec = (f) => (Array.isArray(f[0]) ? f.map((v) => v.map(num)) : f.map(num));

async function main() {
  fa.configure(Object.assign({}, fa._settings, job.settings));
  const clips = job.clips.map((c) => ({ pcm: new Float32Array(fs.readFileSync(c.pcm).buffer.slice(0)), sampleRate: c.fs }));
  const n = clips.length;
  const model = job.model ? fa.loadModel(job.model) : null;
  const out = { stream: { callbacks: clips.map(() => []), preds: [] }, batch: { callbacks: clips.map(() => []), preds: [] } };
  if (model) fa.setPredictionModel(model, (si, lc, s, per) => out.stream.preds.push([si, lc[0], num(lc[1]), s]));
  const h = fa.StreamOpen(n, clips.map((c) => c.sampleRate), (si, label, t, f, s) => out.stream.callbacks[s].push([si, [], t, vec(f)]), [], job.frames_per_step);
  out.stream.handle = { capacity: Array.from(h.capacity), inputStride: h.inputStride, samplesPerStep: h.samplesPerStep };
  const pos = clips.map(() => 0), done = clips.map(() => false);
  let first = true, explicit = 0, paced = 0;
  while (done.some((d) => !d)) {
    // paced: every source delivers what keeps it on real time; a source's last push carries what is left of it and its STOP
    const want = h.paced(), ctl = new Uint8Array(n), counts = new Uint32Array(n);
    let all_paced = true;
    for (let i = 0; i < n; i++) {
      if (done[i]) continue;
      const left = clips[i].pcm.length - pos[i], c = Math.min(want[i], left);
      ctl[i] = fa.STREAM_ACTIVE | (first ? fa.STREAM_START : 0) | (c === left ? fa.STREAM_STOP : 0);
      counts[i] = c;
      if (c !== want[i]) all_paced = false;
      h.input.set(clips[i].pcm.subarray(pos[i], pos[i] + c), i * h.inputStride);
      pos[i] += c;
      if (c === left) done[i] = true;
    }
    if (all_paced) { h.push(ctl); paced++; } else { h.push(ctl, counts); explicit++; }
    first = false;
  }
  h.close();
  out.stream.pushes = { paced, explicit };
  if (model) fa.setPredictionModel(model, (si, lc, clip, per) => out.batch.preds.push([si, lc[0], num(lc[1]), clip]));
  await fa.LaunchBatch(clips, (si, label, t, f, clip) => out.batch.callbacks[clip].push([si, [], t, vec(f)]), [], false);
  fa.setPredictionModel(null);
  process.stdout.write(JSON.stringify(out));
}
main().catch((e) => { console.error(e); process.exit(1); });
