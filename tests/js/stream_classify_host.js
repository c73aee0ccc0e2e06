// stream_classify_host.js — drives js/formantanalyzer.js's StreamOpen with the app's classifier for tests/test_js_host_stream_classify.py.
// usage: node stream_classify_host.js job.json  -> JSON on stdout
//   job = {pcm: f32 file (one signal at fs), fs, settings, model, frames_per_step}
//   out = {batch: {preds, meters}, stream: {preds, callbacks, meters}, plain: {callbacks}, destroy_while_held, destroy_after_close}
'use strict';
const fs = require('fs');
const path = require('path');
const fa = require(path.join(__dirname, '..', '..', 'webspeechanalyzer_amd', 'js', 'formantanalyzer.js'));

const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = {};
const num = (x) => (Number.isFinite(x) ? x : String(x));
const per_of = (per) => (Array.isArray(per[0]) ? per : [per]).map((l) => l.map((e) => [e.label, num(e.confidence)]));

function stream_run(pcm, with_model) {
  const preds = [], cbs = [];
  if (with_model) fa.setPredictionModel(out.h, (si, lc, s, per) => preds.push([si, lc[0], num(lc[1]), s, per_of(per)]));
  else fa.setPredictionModel(null);
  const h = fa.StreamOpen(1, job.fs, (si, label, t, f, s) => cbs.push([si, t, s, f.length]), [], job.frames_per_step);
  const sps = h.samplesPerStep, nsteps = Math.floor(pcm.length / sps);
  for (let k = 0; k < nsteps; k++) {
    h.input.set(pcm.subarray(k * sps, (k + 1) * sps));
    h.push();
  }
  const last = h.close();
  return { preds, callbacks: JSON.stringify(cbs), meters: last.meters || null, used: nsteps * sps };
}

async function main() {
  fa.configure(Object.assign({}, fa._settings, job.settings));
  out.h = fa.loadModel(job.model);
  const raw = new Float32Array(fs.readFileSync(job.pcm).buffer.slice(0));
  const plain = stream_run(raw, false);
  const s = stream_run(raw, true);
  const pcm = raw.slice(0, s.used);
  const preds = [];
  fa.setPredictionModel(out.h, (si, lc, clip, per) => preds.push([si, lc[0], num(lc[1]), clip, per_of(per)]));
  const b = await fa.LaunchBatch([{ pcm, sampleRate: job.fs }], null, [], false);
  fa.setPredictionModel(null);
  out.batch = { preds, meters: b.meters };
  out.stream = { preds: s.preds, callbacks: s.callbacks, meters: s.meters };
  out.plain = { callbacks: plain.callbacks, meters: plain.meters };
  // the addon: a model held by a stream cannot be destroyed; streamClose releases it
  const nat = require(path.join(__dirname, '..', '..', 'webspeechanalyzer_amd', 'lib', 'wsa_napi.node'));
  const d = nat.defaults(); d.output_level = 13;
  const c = nat.create(d, 0);
  const m = nat.modelCreate(c, out.h.spec);
  const st = nat.streamOpen(c, 2, 16000, 1, 1024);
  nat.streamSetModel(st, m);
  try { nat.modelDestroy(m); out.destroy_while_held = 'destroyed'; } catch (e) { out.destroy_while_held = String(e.message || e); }
  nat.streamClose(st);
  try { nat.modelDestroy(m); out.destroy_after_close = 'destroyed'; } catch (e) { out.destroy_after_close = String(e.message || e); }
  nat.destroy(c);
  delete out.h;
  process.stdout.write(JSON.stringify(out));
}
main().catch((e) => { console.error(e); process.exit(1); });
