// stream_knn_host.js — drives js/formantanalyzer.js's StreamOpen and LaunchBatch with a KNN store as the predictor (setPredictionKnn) for
// tests/test_js_host_stream_knn.py.
// usage: node stream_knn_host.js job.json  -> JSON on stdout
//   job = {pcm: f32 file (one signal at fs), fs, settings, store: JSON file {rows: [[53 numbers]], labels: [..]}, k, frames_per_step}
//   out = {stream: {preds, callbacks, meters}, plain: {callbacks, meters}, batch: {preds, meters}, replaced_by_model, step_keys, destroy_while_open}
'use strict';
const fs = require('fs');
const path = require('path');
const fa = require(path.join(__dirname, '..', '..', 'webspeechanalyzer_amd', 'js', 'formantanalyzer.js'));

const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = {};
const num = (x) => (Number.isFinite(x) ? x : String(x));
const per_of = (per) => (Array.isArray(per[0]) ? per : [per]).map((l) => l.map((e) => [e.label, num(e.confidence)]));

function stream_run(pcm, knn) {
  const preds = [], cbs = [];
  if (knn) fa.setPredictionKnn(knn, job.k, (si, lc, s, per) => preds.push([si, lc[0], num(lc[1]), s, per_of(per)]));
  else fa.setPredictionKnn(null);
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
  const store = JSON.parse(fs.readFileSync(job.store, 'utf8'));
  const knn = fa.KNNClassifier(53, store.rows.length);
  knn.addExamples(store.rows, store.labels);
  const raw = new Float32Array(fs.readFileSync(job.pcm).buffer.slice(0));
  const plain = stream_run(raw, null);
  const s = stream_run(raw, knn);
  const pcm = raw.slice(0, s.used);
  const preds = [];
  fa.setPredictionKnn(knn, job.k, (si, lc, clip, per) => preds.push([si, lc[0], num(lc[1]), clip, per_of(per)]));
  const b = await fa.LaunchBatch([{ pcm, sampleRate: job.fs }], null, [], false);
  out.batch = { preds, meters: b.meters };
  out.stream = { preds: s.preds, callbacks: s.callbacks, meters: s.meters };
  out.plain = { callbacks: plain.callbacks, meters: plain.meters };
  // setPredictionModel(null) replaces the store on the JS side: the next launch predicts nothing
  fa.setPredictionModel(null);
  const b2 = await fa.LaunchBatch([{ pcm, sampleRate: job.fs }], null, [], false);
  out.replaced_by_model = b2.meters === undefined && preds.length === out.batch.preds.length;
  // the addon: the step's KNN tables, and a store whose context has an open stream set cannot be destroyed
  const nat = require(path.join(__dirname, '..', '..', 'webspeechanalyzer_amd', 'lib', 'wsa_napi.node'));
  const d = nat.defaults(); d.output_level = 13;
  const c = nat.create(d, 0);
  const ks = nat.knnCreate(c, 53, 4, 8);
  nat.knnAdd(ks, Float64Array.from({ length: 2 * 53 }, (_, i) => 1 + (i % 7)), Int32Array.from([0, 1]));
  const st = nat.streamOpen(c, 2, 16000, 1, 1024);
  nat.streamSetKnn(st, ks, 3);
  out.step_keys = Object.keys(nat.streamStep(st, null)).filter((k) => k.startsWith('knn')).sort();
  try { nat.knnDestroy(ks); out.destroy_while_open = 'destroyed'; } catch (e) { out.destroy_while_open = String(e.message || e); }
  nat.streamSetKnn(st, null);
  out.step_keys_detached = Object.keys(nat.streamStep(st, null)).filter((k) => k.startsWith('knn'));
  nat.streamClose(st);
  nat.knnDestroy(ks);
  nat.destroy(c);
  knn.release();
  process.stdout.write(JSON.stringify(out));
}
main().catch((e) => { console.error(e); process.exit(1); });
