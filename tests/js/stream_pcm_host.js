// stream_pcm_host.js — drives js/formantanalyzer.js's StreamOpen with packed input for tests/test_js_host_stream_pcm.py.
// usage: node stream_pcm_host.js job.json  -> JSON on stdout
//   job = {clips: [{pcm: interleaved i16 file}], fs, channels, settings, frames_per_step}
//   out = {float: {callbacks per source, handle}, i16: {callbacks per source, handle}, g711: {mulaw: [256], alaw: [256]}, refused: [messages]}
'use strict';
const fs = require('fs');
const path = require('path');
const fa = require(path.join(__dirname, '..', '..', 'webspeechanalyzer_amd', 'js', 'formantanalyzer.js'));

const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const num = (x) => (Number.isFinite(x) ? x : String(x));
const vec = (f) => (Array.isArray(f[0]) ? f.map((v) => v.map(num)) : f.map(num));

// every source from START to STOP in whole steps; put(h, i, first frame, frames) writes source i's frames of the step into h.input
function drive(h, n, frames, put) {
  const sps = h.samplesPerStep, steps = Math.floor(frames / sps);
  for (let k = 0; k < steps; k++) {
    const ctl = new Uint8Array(n).fill(fa.STREAM_ACTIVE | (k === 0 ? fa.STREAM_START : 0) | (k === steps - 1 ? fa.STREAM_STOP : 0));
    for (let i = 0; i < n; i++) put(h, i, k * sps, sps);
    h.push(ctl);
  }
  h.close();
}

function main() {
  fa.configure(Object.assign({}, fa._settings, job.settings));
  const ch = job.channels;
  const clips = job.clips.map((c) => new Int16Array(fs.readFileSync(c.pcm).buffer.slice(0)));
  const n = clips.length, frames = Math.min(...clips.map((c) => c.length / ch));
  const out = { float: { callbacks: clips.map(() => []) }, i16: { callbacks: clips.map(() => []) } };
  const floats = clips.map((c) => fa.decodePcm('i16', c, ch));

  let h = fa.StreamOpen(n, job.fs, (si, label, t, f, s) => out.float.callbacks[s].push([si, [], t, vec(f)]), [], job.frames_per_step);
  out.float.handle = { type: h.input.constructor.name, length: h.input.length, samplesPerStep: h.samplesPerStep };
  drive(h, n, frames, (hh, i, j0, c) => hh.input.set(floats[i].subarray(j0, j0 + c), i * hh.samplesPerStep));

  h = fa.StreamOpen(n, job.fs, (si, label, t, f, s) => out.i16.callbacks[s].push([si, [], t, vec(f)]), [], job.frames_per_step, 1024, { format: 'i16', channels: ch });
  out.i16.handle = { type: h.input.constructor.name, length: h.input.length, samplesPerStep: h.samplesPerStep, inputStride: h.inputStride };
  drive(h, n, frames, (hh, i, j0, c) => hh.input.set(clips[i].subarray(j0 * ch, (j0 + c) * ch), i * hh.inputStride));

  const codes = Uint8Array.from({ length: 256 }, (_, i) => i);
  out.g711 = { mulaw: Array.from(fa.decodePcm('mulaw', codes)), alaw: Array.from(fa.decodePcm('alaw', codes)) };
  out.refused = [];
  for (const bad of [() => fa.decodePcm('pcm24', codes), () => fa.decodePcm('mulaw', codes, 65), () => fa.decodePcm('i16', codes),
    () => fa.StreamOpen(n, job.fs, null, [], 1, 1024, { format: 'i16', channels: 0 }), () => fa.StreamOpen(n, job.fs, null, [], 1, 1024, { format: 'f32', channels: 2 })]) {
    try { bad(); out.refused.push(null); } catch (e) { out.refused.push(String(e)); }
  }
  process.stdout.write(JSON.stringify(out));
}
main();
